"""The form for the word that holds one whole two-byte character, without a GPU (word_inside + classify_word_inside of
splintr_amd/csrc/spl_scan_words.h through tests/hostsim/words_inside_sim): called as the classify loop of k_pretok calls it, compared
bit for bit (rec, v0, v1) with the general classify_word.  Whether the form may take a word is decided by the simulation's own byte
loop; where the form declines the test asserts that it had to, and where it takes that it was allowed to.  Three patterns.

  pairs    every lead 0xC0..0xDF x every continuation byte 0x80..0xBF, the lead at byte 0, 1 and 2, every pair of ASCII bytes from one
           representative per ASCII class (apostrophe, space, newline, carriage return, tab, digit, lower, upper, punctuation, '/'),
           each of the 16 values of ts4; the neighbouring words and the text-start bits outside the word change under it
  shapes   every word over ASCII, two-, three- and four-byte leads and continuation bytes, each ts4, each one-byte special-literal span
  places   both sweeps at window index 0 and 4 (with the corpus beginning at, before and behind the word), in the middle, at the last
           full word before the end of the text, at the word that holds the end of the text in each of its bytes, at the window's last word

Two deliberately wrong builds of the form (SPL_WORDS_SIM_BREAK 3: CS on both bytes of the character; 4: ts4 not looked at by the
test) must each be reported."""
import pytest

from words_inside_sim import PATTERNS, TABLES, WordsInsideSim

_sims = {}

# PLACES of tests/hostsim/words_inside_sim.cpp: may the form take a word there at all (the ASCII branch's own edge conditions)?
OPEN = [True, False, True, True, False, True, True, False, False, False, False, False, True]
N_PAIR_WORDS = 32 * 64 * 3 * 10 * 10


def _sim(table=TABLES[0], broken=0):
    if (table, broken) not in _sims:
        _sims[(table, broken)] = WordsInsideSim(table, broken)
    return _sims[(table, broken)]


def _clean(st):
    return st["mismatch"] == 0 and st["declined_wrong"] == 0 and st["took_wrong"] == 0


def test_places_are_what_the_table_says():
    s = _sim()
    assert s.n_places == len(OPEN) and s.n_ascii == 10


@pytest.mark.parametrize("place", range(len(OPEN)))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_pairs(pattern, place):
    st = _sim().sweep("pairs", pattern, place)
    assert st["cases"] == N_PAIR_WORDS * 16
    assert _clean(st), st
    if OPEN[place]:
        # of the 16 values of ts4 the 8 with a text start on the continuation byte are declined, the other 8 taken
        assert st["taken"] == st["declined_ts"] == N_PAIR_WORDS * 8 and st["declined_edge"] == 0 and st["declined_shape"] == 0, st
    else:
        assert st["taken"] == 0 and st["declined_edge"] == st["cases"], st


def test_pairs_other_table():
    st = _sim(TABLES[1]).sweep("pairs", "o200k", 5)
    assert _clean(st) and st["taken"] == N_PAIR_WORDS * 8, st


@pytest.mark.parametrize("place", [0, 1, 5, 6, 10])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_shapes(pattern, place):
    st = _sim().sweep("shapes", pattern, place)
    assert st["cases"] == 9 ** 4 * 16 * 5
    assert _clean(st), st
    # the words of the shape: a lead of 3 (0xC3, 0xD0, 0xC0) and a continuation byte of 2 at 3 offsets, 2 x 2 ASCII bytes around
    shaped = 3 * 2 * 3 * 4
    assert st["declined_shape"] == (9 ** 4 - shaped) * 16 * 5, st
    if OPEN[place]:
        assert st["taken"] == shaped * 8 and st["declined_ts"] == shaped * 8 and st["declined_edge"] == shaped * 16 * 4, st
    else:
        assert st["taken"] == 0 and st["declined_edge"] == shaped * 16 * 5, st


@pytest.mark.parametrize("broken", [3, 4])
def test_broken_variants_are_caught(broken):
    """3: V1_CS also on the continuation byte; 4: a text start on the continuation byte not looked at."""
    st = _sim(TABLES[0], broken).sweep("pairs", "cl100k", 5)
    assert not _clean(st), st
    if broken == 3:
        assert st["mismatch"] == st["taken"] == N_PAIR_WORDS * 8 and st["took_wrong"] == 0, st
    else:
        assert st["took_wrong"] == st["mismatch"] == N_PAIR_WORDS * 8 and st["taken"] == N_PAIR_WORDS * 16, st
    assert not _clean(_sim(TABLES[0], broken).sweep("shapes", "cl100k", 5))
