"""-m gpu: every Unicode scalar value through the device code that decodes UTF-8 and reads the class tables -- the tile kernel's
word classifier (spl_scan_words.h: classify_word, classify_word_two, the CJK short cut, stage1 / stage2 beyond the BMP) in every
execution mode, and the custom-pattern splitter's own look-ups (spl_rx_split.h: cls_of, cat_of, decode, decode_win).

The text is tests/cpsweep.py: every code point in thirteen contexts, at each of the four byte offsets of a 32-bit word, and as a
document of its own (the full sweep), or once (the reduced sweep).  All comparisons are ids and offsets, bit for bit, against the C
oracle, which tests/test_codepoint_sweep_cpu.py pins to PCRE2 over the same sweep; a failure names the code point and the context.
The anchors at the end depend on no oracle: their expectations are data (tests/golden/codepoint_anchors.json)."""
import json
import os

import numpy as np
import pytest

import cpsweep
from conftest import ROOT
from test_gpu_parity import tok

pytestmark = pytest.mark.gpu

FAMILIES = ["cl100k_base", "o200k_base", "mistral_v3"]
DATA = os.path.join(ROOT, "splintr_amd", "data")
ORACLE_THREADS = 16


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _lib():
    from splintr_amd import _ffi
    return _ffi.lib()


def _force(t, mode):
    """spl_debug_phases: 0 by size, 1 tile-owned mode, 4 queue mode, 5 tile-owned mode with the second geometry at any size"""
    import ctypes
    assert _lib().spl_debug_phases(t.handle, mode << 1, (ctypes.c_uint64 * 16)()) == 0


def _packed(docs):
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return b"".join(docs), off


def _compare(t, orc, sweep, what, special=False, want=None):
    """one call on the sweep's documents, one batch, against the C oracle (or its CSR computed before); returns the oracle's CSR"""
    blob, off = _packed(sweep.docs)
    if want is None:
        want = orc.encode_packed(np.frombuffer(blob, dtype=np.uint8), off, special, threads=ORACLE_THREADS)
    got = t.encode_packed(blob, off, with_special=special)
    _same(t, sweep, got, want, what)
    return want


def _same(t, sweep, got, want, what, first_doc=0):
    if not (np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])):
        raise AssertionError(f"{what}: {len(got[0])} ids against the oracle's {len(want[0])}; first difference at "
                             + cpsweep.first_difference(sweep, got, want, t.decode_bytes, first_doc))


_reduced_want = {}


def _reduced(coracle, name):
    """the oracle's CSR of the reduced sweep, computed once per pattern family (callers leave it as it is)"""
    red = cpsweep.reduced_sweep()
    if name not in _reduced_want:
        blob, off = _packed(red.docs)
        _reduced_want[name] = coracle(name).encode_packed(np.frombuffer(blob, dtype=np.uint8), off, False, threads=ORACLE_THREADS)
    return red, _reduced_want[name]


def _blob(name):
    with open(os.path.join(DATA, name + ".splv"), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------------
# the scanner: full sweep by size, reduced sweep in the other modes and forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_full_sweep_in_auto_mode(coracle, name):
    full = cpsweep.full_sweep()
    t = tok(name)
    _force(t, 0)
    _compare(t, coracle(name), full, f"{name}, full sweep ({full.n_bytes} bytes, {len(full.docs)} documents), mode by size")


@pytest.mark.parametrize("mode", [4, 5])
@pytest.mark.parametrize("name", FAMILIES)
def test_reduced_sweep_in_queue_mode_and_the_second_geometry(coracle, name, mode):
    red, want = _reduced(coracle, name)
    t = tok(name)
    _force(t, mode)
    try:
        _compare(t, None, red, f"{name}, reduced sweep, mode {mode}", want=want)
    finally:
        _force(t, 0)


@pytest.mark.parametrize("name", FAMILIES)
def test_reduced_sweep_in_batches_of_one_launch(coracle, name):
    """mode 1 in batches of at most 1 MB: the first geometry (800 + 192), and through the device entry point the ONE-launch form,
    asserted from the launch counts (test_gpu_fused._encode); the same batches through the host path as well"""
    from splintr_amd.device import DeviceBatch
    from test_gpu_fused import _dev, _encode, _profile
    red, want = _reduced(coracle, name)
    w_ids, w_off = want
    t = tok(name)
    edges, size = [0], 0
    for i, d in enumerate(red.docs):
        if size + len(d) > 1_000_000:
            edges.append(i)
            size = 0
        size += len(d)
    edges.append(len(red.docs))
    assert len(edges) > 12
    _force(t, 1)
    _profile(t, True)
    try:
        for a, b in zip(edges[:-1], edges[1:]):
            sub = (w_ids[int(w_off[a]):int(w_off[b])], w_off[a:b + 1] - w_off[a])
            docs = red.docs[a:b]
            for form, got in (("one launch", _encode(t, DeviceBatch([d.decode("utf-8") for d in docs], _dev()), "fused")),
                              ("host path", t.encode_packed(*_packed(docs)))):
                _same(t, red, got, sub, f"{name}, mode 1, {form}, documents {a}..{b}", first_doc=a)
    finally:
        _profile(t, False)
        _force(t, 0)


@pytest.mark.parametrize("name", FAMILIES)
def test_reduced_sweep_as_one_document(coracle, name):
    """13 MB in ONE document: characters straddle every tile edge and every halo edge, no document start resets anything"""
    red = cpsweep.reduced_sweep()
    blob = b"".join(red.docs)
    off = np.array([0, len(blob)], dtype=np.uint64)
    t = tok(name)
    _force(t, 0)
    want = coracle(name).encode_packed(np.frombuffer(blob, dtype=np.uint8), off, False, threads=ORACLE_THREADS)
    got = t.encode_packed(blob, off)
    if not (np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])):
        n = min(len(got[0]), len(want[0]))
        d = np.nonzero(got[0][:n] != want[0][:n])[0]
        k = int(d[0]) if len(d) else n
        byte = len(t.decode_bytes(want[0][:k].tolist()))
        doc = int(np.searchsorted(_packed(red.docs)[1], byte, side="right")) - 1
        raise AssertionError(f"{name}, one document: byte {byte}, {red.describe(doc, byte - int(_packed(red.docs)[1][doc]))}: "
                             f"{got[0][k:k + 6].tolist()} instead of {want[0][k:k + 6].tolist()}")


def test_reduced_sweep_with_the_special_token_flag(coracle):
    """with_special on cl100k_base: the classify path that carries special spans (sk4); every sixteenth document ends in a literal"""
    red = cpsweep.reduced_sweep()
    docs = [d + b"<|endoftext|>" if i % 16 == 0 else d for i, d in enumerate(red.docs)]
    t = tok("cl100k_base")
    _force(t, 0)
    blob, off = _packed(docs)
    want = coracle("cl100k_base").encode_packed(np.frombuffer(blob, dtype=np.uint8), off, True, threads=ORACLE_THREADS)
    assert int((want[0] == 100257).sum()) == len(docs[::16])
    got = t.encode_packed(blob, off, with_special=True)
    _same(t, red, got, want, "cl100k_base, with_special")


# ------------------------------------------------------------------------------------------------
# the second table
# ------------------------------------------------------------------------------------------------
_py_enc = {}


def _py_oracle(name, engine, pattern=None):
    from oracle import pyoracle as O
    if name not in _py_enc:
        _py_enc[name] = O.load_splv(os.path.join(DATA, O.PRETRAINED[name][0]))[0]
    fn, pat, bl = O.PRETRAINED[name]
    return O.Oracle(_py_enc[name], pattern or pat, bl, {}, engine)


def _against_python(t, orc, sweep, what):
    """a sweep against the Python oracle (any engine, any pattern), document by document"""
    blob, off = _packed(sweep.docs)
    ids, o = t.encode_packed(blob, off)
    for d, doc in enumerate(sweep.docs):
        got, want = ids[int(o[d]):int(o[d + 1])].tolist(), orc.encode_bytes(doc)
        if got != want:
            k = next((k for k, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
            raise AssertionError(f"{what}: {sweep.describe(d, min(len(orc.decode_bytes(want[:k])), len(doc) - 1))}: {got[k:k + 6]} instead of {want[k:k + 6]}")


def _differing_code_points():
    from uclassgen import read_table
    a, r = read_table("unicode_classes.bin"), read_table("unicode_classes_regex.bin")
    d = np.nonzero(a.cls != r.cls)[0]
    d = d[(d < 0xD800) | (d > 0xDFFF)]
    assert len(d) > 10000 and 0x180E in d
    return d


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base"])
@pytest.mark.parametrize("engine", ["regex", "pcre2"])
def test_code_points_the_two_tables_class_differently(name, engine):
    """all of them (14 186 with the tables as shipped) in all contexts at all alignments: the table of the `regex` module against
    that engine, the default table against PCRE2"""
    from oracle import pyoracle as O
    from splintr_amd import Tokenizer
    if engine == "regex":
        pytest.importorskip("regex")
        t = Tokenizer.from_pretrained(name, unicode_tables="regex")
    else:
        if not O.pcre2_available():
            pytest.skip("libpcre2-8 not present")
        t = tok(name)
        _force(t, 0)
    sweep = cpsweep.full_contexts(_differing_code_points().tolist())
    _against_python(t, _py_oracle(name, engine), sweep, f"{name}, table and engine {engine}")


# ------------------------------------------------------------------------------------------------
# a table without the CJK short cut
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_table_whose_cjk_ranges_are_not_uniform(tmp_path, name):
    """spl_create accepts any table; every shipped one has U+4E00..U+9FFF and U+AC00..U+D7A3 uniformly Lo, so the branch that
    looks these ranges up (cjk_fast == 0) never ran.  Here the first and the last code point of each range are numbers."""
    from hostsim import HostSim
    from oracle.coracle import COracle
    from splintr_amd import Tokenizer
    from uclassgen import CJK_EDGE_EDITS, CJK_EDGE_KEPT, CLASS_NAMES, read_table, write_edited
    path = str(tmp_path / "unicode_classes_cjk_edges.bin")
    edited = write_edited("unicode_classes.bin", path, CJK_EDGE_EDITS)
    shipped = read_table("unicode_classes.bin")
    assert edited.version == shipped.version == 3
    assert HostSim(name).info()["cjk_fast"] == 1 and HostSim(name, path).info()["cjk_fast"] == 0
    orc = COracle(name, unicode_table=path)
    for cp in CJK_EDGE_EDITS:
        assert orc.class_of(cp) == CLASS_NAMES.index("N") and shipped.cls[cp] == CLASS_NAMES.index("Lo")
    for cp in CJK_EDGE_KEPT:
        assert orc.class_of(cp) == shipped.cls[cp]
    sweep = cpsweep.full_contexts(((0x4D00, 0xA100), (0xAB00, 0xD900)))
    t = Tokenizer.from_pretrained(name, unicode_tables=path)
    want = None
    for mode in (0, 4):
        _force(t, mode)
        want = _compare(t, orc, sweep, f"{name}, table without the CJK short cut, mode {mode}", want=want)
    # (the edit does change the result: the shipped table splits this text differently)
    shipped_ids, _ = tok(name).encode_packed(*_packed(sweep.docs))
    assert len(shipped_ids) != len(want[0]) or not np.array_equal(shipped_ids, want[0])


# ------------------------------------------------------------------------------------------------
# the device splitter of custom patterns
# ------------------------------------------------------------------------------------------------
def _on_the_device(t, docs):
    """the device matcher takes this pattern (its program fits) and gives nothing up on these documents"""
    from test_gpu_device_split import _both
    st, gp, dst, dgp, status = _both(t, docs)
    assert status == 0, f"the device matcher gave up (status {status})"
    assert np.array_equal(st, dst) and np.array_equal(gp, dgp), "the device splitter's bitmaps differ from the host splitter's"


@pytest.mark.parametrize("name", ["cl100k_base"])
def test_device_splitter_on_the_reduced_sweep(coracle, name):
    """cl100k's pattern in a group is another string: it is compiled and run by the device splitter (cls_of, decode, decode_win)"""
    from oracle import pyoracle as O
    from splintr_amd import Tokenizer
    red, want = _reduced(coracle, name)
    t = Tokenizer.from_bytes(_blob(name), "(?:" + O.PRETRAINED[name][1] + ")")
    assert t.has_custom_pattern
    before = _lib().spl_device_split_fallbacks(t.handle)
    _compare(t, None, red, f"{name} in a group, device splitter", want=want)
    assert _lib().spl_device_split_fallbacks(t.handle) == before == 0
    _on_the_device(t, red.docs[:200] + red.docs[-200:])


def _assigned_code_points():
    from uclassgen import GC_NAMES, read_table
    gc = read_table("unicode_classes.bin").gc
    cps = cpsweep.scalar_values(cpsweep.ALL_RANGES)
    cn = cps[gc[cps] == GC_NAMES.index("Cn")]
    return np.sort(np.concatenate([cps[gc[cps] != GC_NAMES.index("Cn")], cn[::64]]))


def _category_pattern():
    from uclassgen import GC_NAMES
    return "|".join(r"\p{%s}+" % n for n in GC_NAMES if n not in ("Cn", "Cs")) + r"|\s+|."


def _script_patterns(per=28):
    from uclassgen import read_table
    names = [n for n, _ in read_table("unicode_classes.bin").scripts]
    assert len(names) > 150
    return ["|".join(r"\p{%s}+" % n for n in names[i:i + per]) + r"|\s+|." for i in range(0, len(names), per)]


_PROPERTY_PATTERNS = ["categories"] + [f"scripts{i}" for i in range(6)]


@pytest.mark.parametrize("which", _PROPERTY_PATTERNS)
def test_device_splitter_reads_categories_and_scripts(which):
    """cat_of and the script ranges: every general category but Cn and Cs, and every script of the table (28 to a pattern: the
    device matcher's first-byte table has a bit per alternative), as alternatives of their own, over every assigned code point and
    every 64th unassigned one, one 'X ' piece each, against the Python oracle on PCRE2"""
    from oracle import pyoracle as O
    from splintr_amd import Tokenizer
    if not O.pcre2_available():
        pytest.skip("libpcre2-8 not present")
    scripts = _script_patterns()
    assert len(scripts) == len(_PROPERTY_PATTERNS) - 1
    pattern = _category_pattern() if which == "categories" else scripts[int(which[7:])]
    sweep = cpsweep.sweep_docs([cpsweep.THIN_CONTEXT], 64, _assigned_code_points().tolist())
    t = Tokenizer.from_bytes(_blob("cl100k_base"), pattern)
    assert t.has_custom_pattern
    before = _lib().spl_device_split_fallbacks(t.handle)
    _against_python(t, _py_oracle("cl100k_base", "pcre2", pattern), sweep, which)
    assert _lib().spl_device_split_fallbacks(t.handle) == before == 0
    _on_the_device(t, sweep.docs[:300])


# ------------------------------------------------------------------------------------------------
# anchors: no oracle
# ------------------------------------------------------------------------------------------------
def _anchors():
    with open(os.path.join(ROOT, "tests", "golden", "codepoint_anchors.json"), encoding="utf-8") as f:
        return {k: v for k, v in json.load(f).items() if not k.startswith("_")}


def test_anchor_expectations_say_what_their_names_say():
    """the recorded PCRE2 splits have the shape that tells the classes apart (no GPU needed for this half, but it belongs here)"""
    a = _anchors()
    assert a["long_s_after_apostrophe"]["pieces"] == ["a", "'\u017f"]              # U+017F is an s under (?i): a contraction
    assert a["kelvin_after_apostrophe"]["pieces"] == ["a", "'\u212a"]              # (k is no contraction letter: the apostrophe is the letters' prefix)
    assert a["u180e_is_whitespace"]["pieces"] == ["\u180e", "!"]                   # punctuation would take the '!' along
    assert a["u180e_run_before_letter"]["pieces"] == ["a", "\u180e", "\u180eb"]     # \s+(?!\S) leaves the last one to the letter
    assert a["u10ffff_then_punctuation"]["pieces"] == ["x", "\U0010ffff!"] and a["ue0001_then_punctuation"]["pieces"] == ["x", "\U000e0001!"]
    assert a["u10ffff_is_other"]["pieces"] == ["x", "\U0010ffffy"] and a["ue0001_is_other"]["pieces"] == ["x", "\U000e0001y"]
    assert a["u2fa1d_is_lo"]["pieces"] == ["a\U0002fa1db"] and a["u2fa1d_between_digits"]["pieces"] == ["1", "\U0002fa1d", "2"]
    for v in a.values():
        assert "".join(v["pieces"]) == v["text"]


@pytest.mark.parametrize("key", sorted(_anchors()))
def test_anchors(key):
    """ids recorded from PCRE2 and the reference's merge; a token never crosses a piece; alone, in a batch and inside a longer text"""
    v = _anchors()[key]
    t = tok("cl100k_base")
    _force(t, 0)
    ids = t.encode(v["text"])
    assert ids == v["ids"], (key, ids, v["ids"])
    cuts, at = set(), 0
    for i in ids:
        at += len(t.decode_bytes([i]))
        cuts.add(at)
    want, at = set(), 0
    for p in v["pieces"]:
        at += len(p.encode("utf-8"))
        want.add(at)
    assert want <= cuts, (key, sorted(want), sorted(cuts))
    batch = t.encode_batch(["lorem ipsum.\n" * k + v["text"] for k in range(0, 200)])      # (every offset mod 4, several tiles)
    for k, got in enumerate(batch):
        assert got[len(got) - len(ids):] == ids, (key, k)
