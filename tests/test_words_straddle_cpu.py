"""The form for the two words that one two-byte character straddles, without a GPU (straddle_shape + word_straddle +
classify_word_straddle of splintr_amd/csrc/spl_scan_words.h through tests/hostsim/words_straddle_sim): called as the classify loop of
k_pretok calls it, on BOTH words of the pair -- the one with the lead in byte 3, the one with the continuation in byte 0 --, compared
bit for bit (rec, v0, v1) with the general classify_word.  Whether the form may take a word is decided by the simulation's own byte
loop; where the form declines the test asserts that it had to, and where it takes that it was allowed to.  Three patterns.

  pairs    every lead 0xC0..0xDF x every continuation byte 0x80..0xBF, every pair of ASCII bytes directly before the lead and directly
           behind the continuation from one representative per ASCII class (apostrophe, space, newline, carriage return, tab, digit,
           lower, upper, punctuation, '/'), a text start on the lead and on the continuation byte (window index i0 + 4) in their four
           combinations; the other bytes of both words, the far words and the text-start bits outside the pair change under it
  starts   every ts4 of both words (256 combinations) over four characters and four ASCII bytes either side, the text-start bits
           outside the pair none and all
  shapes   the four bytes at the boundary over ASCII, two-, three- and four-byte leads and continuation bytes, the outer bytes of both
           words ASCII or not, a special-literal span on the boundary's bytes and on the pair's outer bytes
  places   the lead word as the window's first word with the corpus beginning at it and two, three, four bytes behind it; the
           continuation word as the window's first word; the middle; the lead word as the window's last staged word; the lead word as
           the last full word before the end of the text, with the text ending ON the lead's word end (iB = 40), right behind the
           continuation byte (41), and a word later (44)

The shares of taken words below follow from the sweeps' construction (stated at each assertion); they are the condition that the
test tests something.  Two deliberately wrong builds of the form (SPL_WORDS_SIM_BREAK 5: CS also on the continuation byte; 6: the text
start on the continuation byte not looked at) must each be reported."""
import pytest

from words_straddle_sim import PATTERNS, TABLES, WordsStraddleSim

_sims = {}

# PLACES of tests/hostsim/words_straddle_sim.cpp: (the lead word may be taken there, the continuation word may, words of the pair that
# the loop classifies at all)
OPEN = [(True, True, 2), (False, True, 2), (False, True, 2), (False, False, 2), (False, False, 1), (True, True, 2), (False, False, 1),
        (False, False, 2), (True, False, 2), (True, True, 2)]
N_PAIRS = 32 * 64 * 10 * 10 * 4
N_STARTS = 4 * 4 * 4 * 256 * 2


def _sim(table=TABLES[0], broken=0):
    if (table, broken) not in _sims:
        _sims[(table, broken)] = WordsStraddleSim(table, broken)
    return _sims[(table, broken)]


def _clean(st):
    return st["mismatch"] == 0 and st["declined_wrong"] == 0 and st["took_wrong"] == 0


def test_places_are_what_the_table_says():
    s = _sim()
    assert s.n_places == len(OPEN) and s.n_ascii == 10


def _check_counts(st, n, place):
    """n pairs, every one of the shape; half of them with a text start on the continuation byte: each OPEN word of the pair is taken in
    the other half and declined for the text start in this one; a word that is not open is declined for its edge every time."""
    lead, cont, words = OPEN[place]
    assert st["cases"] == n * words and st["inside"] == 0 and st["declined_shape"] == 0, st
    assert st["taken_lead"] == (n // 2 if lead else 0) and st["taken_cont"] == (n // 2 if cont else 0), st
    assert st["declined_ts"] == (n // 2) * (lead + cont) and st["declined_edge"] == n * (words - lead - cont), st


@pytest.mark.parametrize("place", range(len(OPEN)))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_pairs(pattern, place):
    st = _sim().sweep("pairs", pattern, place)
    assert _clean(st), st
    _check_counts(st, N_PAIRS, place)


@pytest.mark.parametrize("place", range(len(OPEN)))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_starts(pattern, place):
    st = _sim().sweep("starts", pattern, place)
    assert _clean(st), st
    _check_counts(st, N_STARTS, place)


def test_pairs_other_table():
    st = _sim(TABLES[1]).sweep("pairs", "o200k", 5)
    assert _clean(st) and st["taken_lead"] == st["taken_cont"] == N_PAIRS // 2, st


@pytest.mark.parametrize("place", range(len(OPEN)))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_shapes(pattern, place):
    st = _sim().sweep("shapes", pattern, place)
    lead, cont, words = OPEN[place]
    assert st["cases"] == 9 ** 4 * 3 * 3 * 4 * 5 * words
    assert _clean(st), st
    # the words of a side's shape: the word's three other bytes ASCII (1 outer x 2), a two-byte lead of 3 (0xC3, 0xD0, 0xC0), a
    # continuation byte of 2, the boundary's fourth byte (9) and the other word's outer bytes (3) free; each with 4 text-start
    # combinations and 5 spans, of which "none" and "the other word's far byte" leave the word open
    shaped = 1 * 2 * 3 * 2 * 9 * 3
    assert st["taken_lead"] == (shaped * 2 * 2 if lead else 0) and st["taken_cont"] == (shaped * 2 * 2 if cont else 0), st
    assert st["declined_ts"] == shaped * 2 * 2 * (lead + cont), st
    assert st["declined_edge"] == shaped * 4 * (3 * (lead + cont) + 5 * (words - lead - cont)), st


@pytest.mark.parametrize("broken", [5, 6])
def test_broken_variants_are_caught(broken):
    """5: V1_CS also on the continuation byte (the continuation word's byte 0); 6: a text start on the continuation byte not looked at."""
    st = _sim(TABLES[0], broken).sweep("pairs", "cl100k", 5)
    assert not _clean(st), st
    if broken == 5:
        assert st["mismatch"] == st["taken_cont"] == N_PAIRS // 2 and st["took_wrong"] == 0, st
    else:
        assert st["took_wrong"] == st["mismatch"] == N_PAIRS and st["taken_lead"] == st["taken_cont"] == N_PAIRS, st
    assert not _clean(_sim(TABLES[0], broken).sweep("starts", "cl100k", 5))
    assert not _clean(_sim(TABLES[0], broken).sweep("shapes", "cl100k", 5))
