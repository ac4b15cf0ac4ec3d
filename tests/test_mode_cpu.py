"""Which mode a device call runs in, without a GPU: pick_mode and the three size limits (splintr_amd/csrc/spl_mode.h, through
tests/hostsim/mode_sim) against the table written out by hand below -- every force_tile value of spl_debug_phases, with and without
external chunk boundaries, with and without the GPU's special-token scan, at both sides of every limit."""
import pytest

import mode_sim

A_MAX = 1280 * 1024                     # tile-owned geometry A up to here, B beyond
DIRECT_MAX = 256 << 20                  # the tile-owned mode ends here
QUEUE_MAX = 2047 << 20                  # ... and queue mode here
SIZES = (0, 1, A_MAX, A_MAX + 1, DIRECT_MAX, DIRECT_MAX + 1, QUEUE_MAX, QUEUE_MAX + 1)

# one letter per size of SIZES -- A / B: tile-owned in that geometry, Q: queue mode, R: refused
BY_SIZE = "AAABBRRR"                    # tile-owned by size, nothing beyond it
ALL_B = "BBBBBRRR"                      # geometry B forced
NONE = "RRRRRRRR"
TABLE = {
    # (ext, special): one row per force_tile 0 .. 5
    (False, False): ["AAABBQQR",        # 0: by size, queue mode where the tile-owned mode ends
                     BY_SIZE,           # 1: tile-owned only
                     NONE, NONE,        # 2, 3: only run with external boundaries
                     "AQQQQQQR",        # 4: queue mode wherever it has a form (a call without a byte launches no tile: tile-owned)
                     ALL_B],
    # the special-token scan has no form in queue mode
    (False, True): [BY_SIZE, BY_SIZE, NONE, NONE, BY_SIZE, ALL_B],
    # external boundaries: tile-owned whatever is forced, never queue mode
    (True, False): [BY_SIZE, BY_SIZE, BY_SIZE, BY_SIZE, BY_SIZE, ALL_B],
    (True, True): [BY_SIZE, BY_SIZE, BY_SIZE, BY_SIZE, BY_SIZE, ALL_B],
}


def test_limits():
    assert mode_sim.limits() == (A_MAX, DIRECT_MAX, QUEUE_MAX)


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("force_tile", [0, 1, 2, 3, 4, 5])
def test_pick_mode_table(force_tile, ext, special):
    want = TABLE[(ext, special)][force_tile]
    assert len(want) == len(SIZES)
    got = "".join(mode_sim.pick(force_tile, ext, special, n) for n in SIZES)
    assert got == want, (force_tile, ext, special)
