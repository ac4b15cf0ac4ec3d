"""SentencePiece mode without a GPU: the per-tile logic the kernel runs (csrc/spl_k_sp.h through tests/hostsim/sp_sim.cpp) against the
restated reference loop (tests/sp_ref.py) -- rewritten text, chunk starts and document offsets; tiles of 64 and 128 bytes so that a
seam falls into every kind of run."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))
import sp_ref  # noqa: E402
import sp_sim  # noqa: E402


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("name", sorted(sp_sim.CASES))
def test_rewrite_matches_reference(name, tile):
    texts = sp_sim.CASES[name]
    special = sp_sim.SPECIAL if name == "specials" else None
    assert sp_sim.rewrite(texts, tile, special) == sp_ref.rewrite(texts, special)


@pytest.mark.parametrize("shift", range(0, 70, 7))
def test_every_alignment_of_a_mixed_text(shift):
    """One text with every kind of run, pushed byte by byte over the 64-byte seams."""
    texts = ["q" * shift + " a  \n  ab \u00a0 b \u3000 x\x0b  y   " * 5]
    assert sp_sim.rewrite(texts) == sp_ref.rewrite(texts)
