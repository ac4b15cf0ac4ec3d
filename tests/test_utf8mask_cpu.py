"""UTF-8 continuation masks without a GPU: the rule (tests/utf8_mask_ref.py) pinned by hand-worked examples, by Python's own decoder and by
the hold-mode decoders of splintr_amd.streaming -- a bit is 1 iff feeding the id does not stall the decoder --, and the code the kernels
run (splintr_amd/csrc/spl_k_utf8mask.h, evaluated by tests/hostsim/utf8mask_sim.cpp over spl_k_heal.h's wave policy) against that rule:
the automaton byte by byte, the class of every state word, the class table word for word, the row gather with poisoned destinations."""
import itertools
import random

import numpy as np
import pytest

import utf8_mask_ref as ref
from stream_ref import _can_complete

from splintr_amd.streaming import StreamingDecoder


@pytest.fixture(scope="module")
def sim():
    import utf8mask_sim
    utf8mask_sim.lib()
    return utf8mask_sim


@pytest.fixture(scope="module")
def toy():
    vocab, specials = ref.toy()
    assert len(set(vocab.values())) == len(vocab), "the toy vocabulary names a byte string twice"
    return vocab, specials


# ---------------------------------------------------------------------------------------------- the rule, by hand
def test_ref_by_hand():
    ok = [b"", b"a", "é".encode(), b"\xc3", b"a\xe2\x82", "€".encode() + b"\xf0\x9f\x98", b"\xf4\x8f\xbf\xbf", b"\xed\x9f\xbf", b"\xe0\xa0", b"\xf0\x90"]
    bad = [b"\x80", b"\xc0\x80", b"\xc1", b"\xf5", b"\xff", b"\xc3a", b"\xe0\x9f", b"\xed\xa0", b"\xf0\x8f", b"\xf4\x90", b"\xe2\x82a", b"a\x80", b"\xc3\xc3"]
    assert all(ref.prefix_valid(b) for b in ok) and not any(ref.prefix_valid(b) for b in bad)
    assert [ref.pending_class(p) for p in ref.CLASS_REPS] == list(range(8))
    assert ref.pending_class(b"\xe1\x80") == 1 and ref.pending_class(b"\xf0\x90") == 2 and ref.pending_class(b"\xf4\x8f\xbf") == 1
    assert not ref.is_beginning(b"a") and not ref.is_beginning(b"\xc3\xa9") and not ref.is_beginning(b"\xe0\x80") and ref.is_beginning(b"\xe0")
    vocab = {0: b"a", 1: b"\xc3", 2: b"\xa9", 3: "é".encode(), 5: b"", 6: b"\xa9\xff"}
    specials = {4: b"<s>", 9: b"<e>"}
    assert ref.allowed(vocab, specials, b"") == {0, 1, 3, 4, 5, 9}
    assert ref.allowed(vocab, specials, b"\xc3") == {2, 5}
    assert ref.allowed(vocab, specials, b"\xc3", skip=True) == {2, 4, 5, 9}
    row, live = ref.mask_row(vocab, specials, ref.state_word(b"\xc3"), True, 2)
    assert row.tolist() == [0x234, 0] and live == 1
    row, live = ref.mask_row(vocab, specials, ref.state_word(stalled=True, held=9), False, 2)
    assert row.tolist() == [0xFFFFFFFF] * 2 and live == 0


def test_ref_against_pythons_decoder():
    """every string of up to three bytes over the edges of the table, and every pair of bytes"""
    edges = [0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF]
    for n in range(0, 4):
        for t in itertools.product(edges, repeat=n):
            b = bytes(t)
            assert ref.prefix_valid(b) == ref._py_valid(b), b
    for t in itertools.product(range(256), repeat=2):
        assert ref.prefix_valid(bytes(t)) == ref._py_valid(bytes(t)), t
    rng = random.Random(5)
    for _ in range(20000):
        b = bytes(rng.choice(edges) for _ in range(rng.randrange(4, 9)))
        assert ref.prefix_valid(b) == ref._py_valid(b), b


def test_ref_is_the_hold_mode_decoder(toy):
    """a bit is 1 iff a hold-mode decoder brought to that pending state and fed that id does not stall"""
    vocab, specials = toy
    known = dict(specials)
    known.update(vocab)
    for label, word in ref.toy_states():
        if word & ref.STALLED:
            continue
        n = (word >> 24) & 3
        p = (word & 0xFFFFFF).to_bytes(3, "little")[:n]
        ok = ref.allowed(vocab, specials, p)
        for t, b in known.items():
            dec = StreamingDecoder(known.get)
            dec._buf += p                                  # (what the decoder holds in this state)
            dec.add_token(t)
            buf = bytes(dec._buf)
            stalled = bool(buf) and not _can_complete(buf)
            assert stalled == (t not in ok), (label, t, b)


def test_class_table_judge_is_the_rule(toy):
    vocab, specials = toy
    known = dict(specials)
    known.update(vocab)
    nw = max(known) // 32 + 1
    tab = ref.class_table(sorted(known.items()), nw)
    for c, p in enumerate(ref.CLASS_REPS):
        want, _ = ref.mask_row(vocab, specials, ref.state_word(p), False, nw)
        assert (tab[c] == want).all(), c


# ---------------------------------------------------------------------------------------------- the kernels' code: automaton and classes
def test_step_of_every_state_and_byte(sim):
    for s in range(8):
        for x in range(256):
            p = ref.CLASS_REPS[s] + bytes([x])
            got = sim.step(s, x)
            if not ref.prefix_valid(p):
                assert got == 8, (s, x)
            elif ref.is_beginning(p):
                assert got == ref.pending_class(p), (s, x)
            elif s == 0:
                assert got == 0 and x < 0x80, (s, x)
            else:
                assert got == 0 and ref.pending_class(ref.CLASS_REPS[s]) == 1, (s, x)
    assert sim.step(8, 0x41) == 8 and sim.step(9, 0x80) == 8


def test_class_of_every_state_word(sim):
    for label, word in ref.toy_states():
        if word & ref.STALLED:
            assert sim.state_class(word) == sim.FREE, label
        else:
            n = (word >> 24) & 3
            assert sim.state_class(word) == ref.pending_class((word & 0xFFFFFF).to_bytes(3, "little")[:n]), label
    # every pending string of one and two bytes, and three-byte ones over the edges: a word no decoder leaves is free
    edges = [0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC1, 0xC2, 0xE0, 0xED, 0xEF, 0xF0, 0xF4, 0xF5]
    cases = [bytes(t) for n in (1, 2) for t in itertools.product(range(256), repeat=n)] + [bytes(t) for t in itertools.product(edges, repeat=3)]
    for p in cases:
        want = ref.pending_class(p) if ref.is_beginning(p) else sim.FREE
        assert sim.state_class(ref.state_word(p)) == want, p
    assert sim.state_class(ref.state_word(stalled=True) | 0xC3 | (1 << 24)) == sim.FREE


def test_token_classes_against_the_rule(sim, toy):
    vocab, _ = toy
    rng = random.Random(11)
    edges = [0x41, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC2, 0xE0, 0xE1, 0xED, 0xF0, 0xF1, 0xF4, 0xF5]
    toks = list(vocab.values()) + [bytes(rng.choice(edges) for _ in range(rng.randrange(0, 9))) for _ in range(4000)]
    for b in toks:
        want = sum(1 << c for c, p in enumerate(ref.CLASS_REPS) if ref.prefix_valid(p + b))
        assert sim.token_classes(b) == want, b


# ---------------------------------------------------------------------------------------------- the table and the gather
@pytest.fixture(scope="module")
def toy_table(sim, toy):
    vocab, specials = toy
    v = sim.Vocab(vocab, specials)
    return v, sim.table(v)


def test_table_word_for_word(sim, toy, toy_table):
    vocab, specials = toy
    v, rows = toy_table
    assert rows.shape == (17, v.stride) and v.stride % 4 == 0 and v.min_words == max(max(vocab), max(specials)) // 32 + 1
    only_sp = {t: b for t, b in specials.items() if t not in vocab}
    for c, p in enumerate(ref.CLASS_REPS):
        want_v, _ = ref.mask_row(vocab, {}, ref.state_word(p), False, v.stride)
        want_s, _ = ref.mask_row(only_sp, {}, ref.state_word(p), False, v.stride)
        assert (rows[c] == want_v).all() and (rows[8 + c] == want_s).all(), c
    any_sp = np.zeros(v.stride * 32, dtype=np.uint8)
    any_sp[list(only_sp)] = 1
    assert (rows[16] == np.packbits(any_sp, bitorder="little").view(np.uint32)).all()
    assert (rows[0, ref.toy_empty_id() >> 5] >> (ref.toy_empty_id() & 31)) & 1       # the empty token: allowed from the start ...
    assert all((rows[c, ref.toy_empty_id() >> 5] >> (ref.toy_empty_id() & 31)) & 1 for c in range(8))      # ... and in every state


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("per", [1, 4])
def test_masks_of_every_state(sim, toy, toy_table, skip, per):
    vocab, specials = toy
    v, rows = toy_table
    words = [w for _, w in ref.toy_states()]
    for n_words in (v.min_words, v.min_words + 1, 2 * v.min_words):
        if per == 4 and n_words % 4:
            continue
        want, want_live = ref.masks(vocab, specials, words, skip, n_words)
        got, live = sim.run(rows, words, skip=skip, n_words=n_words, per=per)
        assert (got == want).all() and (live == want_live).all(), n_words
        top = max(max(vocab), max(specials)) + 1
        bits = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")
        assert (bits[want_live == 1][:, top:] == 0).all()                       # the bits beyond the largest known id


def test_and_into_and_no_live(sim, toy, toy_table):
    vocab, specials = toy
    v, rows = toy_table
    words = [w for _, w in ref.toy_states()]
    nw = v.min_words + 3
    rng = np.random.default_rng(3)
    other = rng.integers(0, 1 << 32, size=(len(words), nw), dtype=np.uint64).astype(np.uint32)
    want, _ = ref.masks(vocab, specials, words, False, nw)
    got, _ = sim.run(rows, words, and_into=other, n_words=nw)
    assert (got == (want & other)).all()
    got, _ = sim.run(rows, words, n_words=nw, want_live=False)
    assert (got == want).all()
    got, live = sim.run(rows, [], n_words=nw)
    assert got.shape == (0, nw) and live.shape == (0,)


def test_self_check_under_host_sanitizers(tmp_path):
    """the simulation's own main(), a stand-alone program, built with AddressSanitizer and UBSan: the kernels' first half reads and writes
    nothing it should not"""
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "utf8mask_sim.cpp")
    exe = str(tmp_path / "utf8mask_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-unknown-pragmas", "-DUTF8MASK_SIM_MAIN", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "utf8mask_sim: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-1500:])
