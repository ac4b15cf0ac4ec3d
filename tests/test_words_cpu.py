"""The two-byte form of the word classifier, without a GPU (splintr_amd/csrc/spl_scan_words.h through tests/hostsim/words_sim):
classify_word_text -- which tries classify_word_two first -- against the general classify_word, bit for bit (rec, v0, v1), and
classify_word_two called directly: it takes every word whose bytes beyond ASCII are whole two-byte characters (so the comparison
cannot pass by declining) and declines every other one.  Three patterns, both class tables.

  positions   every code point U+0080..U+07FF and the overlong forms behind 0xC0 / 0xC1, the lead at byte 3 of the word before and at
              bytes 0..3 of the word, every neighbour (ASCII letter, digit, space, newline, apostrophe, '/', a two-, three- and
              four-byte character, a stray continuation byte, a lead without its continuation) in front and behind
  fillings    every filling of the word with two and three two-byte characters of different classes and ASCII between them
  guards      every text-start bit alone, lo and iT at the guard's edges

The positions also run on a build without the sub-case for "one character touches the word" (SPL_WORD_TWO_ONE=0), so that the form
for up to three characters sees every single character too.  Two deliberately wrong builds of the header (SPL_WORDS_SIM_BREAK) must each be reported by the same sweeps."""
import pytest

from words_sim import PATTERNS, SWEEPS, TABLES, WordsSim

_sims = {}


def _sim(table, broken=0):
    if (table, broken) not in _sims:
        _sims[(table, broken)] = WordsSim(table, broken)
    return _sims[(table, broken)]


def _clean(st):
    return (st["mismatch"] == 0 and st["two_mismatch"] == 0 and st["declined_well_formed"] == 0 and st["took_malformed"] == 0
            and st["guard_violation"] == 0)


@pytest.mark.parametrize("form", [0, "full"])          # with the sub-case of one character (the product), and every word through the full form
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_positions(pattern, table, form):
    st = _sim(table, form).sweep("positions", pattern)
    assert st["cases"] == 32 * 64 * 5 * 11 * 11
    assert _clean(st), st
    # the two-byte form took every well-formed word, and well-formed and malformed words are both there in number
    assert st["well_formed"] > 400000 and st["malformed"] > 400000 and st["overlong"] > 20000, st
    assert st["two_taken"] == st["well_formed"] + st["overlong_taken"], st
    assert st["text_done"] >= st["two_taken"], st


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_fillings(pattern, table):
    st = _sim(table).sweep("fillings", pattern)
    assert _clean(st), st
    # every filling is well-formed whatever stands at the two bytes next to it; three characters touch the word in one tiling only,
    # [C L C L] + C with its first lead in the word before: 12 characters cubed, 3 x 3 bytes around
    assert st["malformed"] == 0 and st["overlong"] == 0 and st["chars3"] == 12 ** 3 * 9 and st["chars2"] > 100000, st
    assert st["two_taken"] == st["well_formed"] == st["text_done"] == st["cases"], st


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_guards(pattern, table):
    st = _sim(table).sweep("guards", pattern)
    assert _clean(st), st
    # per base word: 16 text-start bits (6 outside the guarded range), 5 values of lo (3 allowed), 5 of iT (3 allowed), i0 = 3 and 2
    assert st["cases"] == 6 * (16 + 5 + 5 + 2)
    assert st["two_taken"] == st["well_formed"] == st["text_done"] == 6 * (6 + 3 + 3 + 1), st


def test_named_words():
    """A few words by hand: what the sweeps count is what it should be."""
    s = _sim(TABLES[0])
    E = b"\xC3\xA9"
    for b, taken in ((b"xxxx" + b"caf\xC3" + b"\xA9xxx", True),                  # the lead in byte 3, its continuation in the next word
                     (b"xxx\xC3" + b"\xA9 et" + b"xxxx", True),                  # the continuation in byte 0, its lead in the word before
                     (b"xxxx" + E + E + b"xxxx", True),                           # [L C L C]
                     (b"xxx\xD0" + b"\xB6\xD0\xB6\xD0" + b"\xB6xxx", True),      # [C L C L] + C: three characters
                     (b"xxxx" + b"a\xE2\x80\x94" + b"xxxx", False),              # a three-byte character
                     (b"xx\xE2\x80" + b"\x94abc" + b"xxxx", False),              # ... its last byte in byte 0
                     (b"xxxx" + b"a\xA9bc" + b"xxxx", False),                    # a stray continuation byte
                     (b"xxxx" + b"a\xC3bc" + b"xxxx", False),                    # a lead without its continuation
                     (b"xxxx" + b"abc\xC3" + b"xxxx", False),                    # ... in byte 3
                     (b"xxxa" + b"\xA9abc" + b"xxxx", False),                    # a continuation in byte 0 whose lead is not byte 3 of the word before
                     (b"xxxx" + E + b"\xA9a" + b"xxxx", False),                  # a second continuation byte
                     (b"xxxx" + b"\xC3\xC3\xA9a" + b"xxxx", False)):             # lead behind lead
        text, general, two = s.one("cl100k", b)
        assert (two is not None) == taken, b
        assert text is None or text == general, b                                # (declined by both forms: the general path's)
        assert text is not None or not taken, b
        if taken:
            assert two == general, b
    # the record of "caf" + lead: three ASCII letters and a lead of a two-byte lower-case letter; CS on all four bytes, no BAD
    text, general, two = s.one("cl100k", b"xxxx" + b"caf\xC3" + b"\xA9xxx")
    assert two[0] >> 24 == (1 << 6) | (general[0] >> 24 & 0xF) and two[2] & 0xFF == 0x0F


@pytest.mark.parametrize("broken", [1, 2])
def test_broken_variants_are_caught(broken):
    """1: V1_CS also on the continuation byte; 2: a continuation in byte 0 accepted without looking at the word before."""
    caught = []
    for sweep in SWEEPS:
        st = _sim(TABLES[0], broken).sweep(sweep, "cl100k")
        caught.append(not _clean(st))
    assert caught[0], caught                                                     # (the fillings are all well-formed: only variant 1 shows there)
    assert caught[1] == (broken == 1), caught
    st = _sim(TABLES[0], broken).sweep("positions", "cl100k")
    if broken == 1:
        assert st["mismatch"] > 0 and st["two_mismatch"] > 0 and st["took_malformed"] == 0, st
    else:
        assert st["took_malformed"] > 0 and st["mismatch"] > 0, st
