"""The code-point space on the CPU (no GPU): (a) the two committed class tables equal what their engines say about every code
point -- classes, caseless partners of the contraction letters, general categories, scripts --; (b) the C oracle, which reads
the same table as the kernels, splits the full sweep (tests/cpsweep.py: every code point in every context at every alignment)
exactly as PCRE2 does; (c) the host compile of the scanner headers splits the reduced sweep as the oracle does, tiled like the
kernel.  With (a) and (b) the oracle side of tests/test_gpu_codepoint_sweep.py is pinned to the engine, not to the table."""
import importlib.util
import os
import time
import warnings

import numpy as np
import pytest

import cpsweep
from conftest import ROOT
from uclassgen import CLASS_NAMES, GC_NAMES, N_CP, read_table, table_bytes

PATTERNS = ["cl100k_base", "o200k_base", "mistral_v3"]
FOLD_LETTERS = "stremvld"


# ------------------------------------------------------------------------------------------------
# (a) the tables equal their engines
# ------------------------------------------------------------------------------------------------
class _Probe:
    """member sets of a pattern over the string of all scalar values, as a boolean array over code points"""

    def __init__(self, engine):
        self.engine = engine
        self.cps = cpsweep.scalar_values(cpsweep.ALL_RANGES)
        if engine == "pcre2":
            from oracle import pyoracle as O
            self.O = O
            arr = self.cps.astype("<u4")
            self.data = arr.tobytes().decode("utf-32-le").encode("utf-8")
            self.start = np.concatenate([[0], np.cumsum(cpsweep.utf8_len(self.cps))])
        else:
            self.regex = pytest.importorskip("regex")
            self.text = self.cps.astype("<u4").tobytes().decode("utf-32-le")

    def members(self, pattern):
        """code points inside any match of `pattern` (runs of members are one match: use \\p{..}+)"""
        if self.engine == "pcre2":
            spans = np.asarray(self.O.Pcre2Pattern(pattern).find_iter(self.data), dtype=np.int64).reshape(-1, 2)
            a, b = np.searchsorted(self.start, spans[:, 0]), np.searchsorted(self.start, spans[:, 1])
        else:
            spans = np.asarray([m.span() for m in self.regex.finditer(pattern, self.text)], dtype=np.int64).reshape(-1, 2)
            a, b = spans[:, 0], spans[:, 1]
        d = np.zeros(len(self.cps) + 1, dtype=np.int64)
        np.add.at(d, a, 1)
        np.add.at(d, b, -1)
        out = np.zeros(N_CP, dtype=bool)
        out[self.cps] = np.cumsum(d[:-1]) > 0
        return out

    def knows(self, pattern):
        try:
            return self.members(pattern)
        except Exception:
            return None


def _engine_or_skip(engine, table):
    """the probe, if the engine on this machine is the version the table's header names"""
    if engine == "pcre2":
        from oracle import pyoracle as O
        if not O.pcre2_available():
            pytest.skip("libpcre2-8 not present")
        have = O.pcre2_versions()[1]
    else:
        regex = pytest.importorskip("regex")
        have = "regex-" + regex.__version__[:9]
    if have.encode()[:16] != table.unicode_version.rstrip(b"\0"):
        pytest.skip(f"the table was probed from {table.engine_version!r}, this machine has {have!r}")
    return _Probe(engine)


def _differ(name, got, want):
    d = np.nonzero(got != want)[0]
    assert not len(d), f"{name}: {len(d)} code points differ from the engine, first U+{int(d[0]):04X} (table {bool(got[d[0]])}, engine {bool(want[d[0]])})"


TABLES = [("unicode_classes.bin", "pcre2"), ("unicode_classes_regex.bin", "regex")]


@pytest.fixture(scope="module", params=TABLES, ids=[e for _, e in TABLES])
def table_and_probe(request):
    fn, engine = request.param
    t = read_table(fn)
    assert t.version == 3 and t.shift == 7
    return fn, t, _engine_or_skip(engine, t)


def test_table_file_is_what_its_two_stage_tables_say(table_and_probe):
    """the reader and the writer of tests/uclassgen.py agree with the file byte for byte: nothing truncated, nothing behind the end"""
    fn, t, _ = table_and_probe
    with open(os.path.join(ROOT, "splintr_amd", "data", fn), "rb") as f:
        assert table_bytes(t) == f.read()


def test_classes_equal_the_engine(table_and_probe):
    _, t, p = table_and_probe
    want = np.zeros(N_CP, dtype=np.uint8)                       # P: what no probe claims (surrogates too: never seen in UTF-8)
    claimed = np.zeros(N_CP, dtype=bool)
    for name in ("Lu", "Ll", "Lt", "Lm", "Lo", "M", "N"):
        m = p.members(r"\p{%s}+" % name)
        assert not (m & claimed).any(), name
        claimed |= m
        want[m] = CLASS_NAMES.index(name)
    ws = p.members(r"\s+")
    assert not (ws & claimed).any()
    want[ws] = CLASS_NAMES.index("WS")
    assert ws[0x20] and ws[0x0A] and ws[0x0D]
    want[0x20], want[0x0A], want[0x0D], want[0x27] = (CLASS_NAMES.index(n) for n in ("SP", "NL", "NL", "AP"))
    d = np.nonzero(t.cls != want)[0]
    assert not len(d), (f"{len(d)} code points are classed differently by the engine, first U+{int(d[0]):04X}: "
                        f"table {CLASS_NAMES[t.cls[d[0]]]}, engine {CLASS_NAMES[want[d[0]]]}")
    # the sets the patterns use, probed as the patterns write them
    L = (t.cls >= CLASS_NAMES.index("Lu")) & (t.cls <= CLASS_NAMES.index("Lo"))
    N = t.cls == CLASS_NAMES.index("N")
    S = (t.cls >= CLASS_NAMES.index("SP")) & (t.cls <= CLASS_NAMES.index("NL"))
    valid = np.zeros(N_CP, dtype=bool)
    valid[p.cps] = True
    _differ(r"\p{L}", L, p.members(r"\p{L}+"))
    _differ(r"[^\s\p{L}\p{N}]", valid & ~L & ~N & ~S, p.members(r"[^\s\p{L}\p{N}]+"))
    nl = np.zeros(N_CP, dtype=bool)
    nl[[0x0A, 0x0D]] = True
    _differ(r"[^\r\n\p{L}\p{N}]", valid & ~L & ~N & ~nl, p.members(r"[^\r\n\p{L}\p{N}]+"))
    _differ(r"\S", valid & ~S, p.members(r"\S+"))


def test_fold_list_equals_the_engine(table_and_probe):
    _, t, p = table_and_probe
    want = []
    for ch in FOLD_LETTERS:
        want += [(int(cp), ord(ch)) for cp in np.nonzero(p.members(f"(?i:{ch})"))[0]]
    assert sorted(t.folds) == sorted(want), (sorted(set(t.folds) ^ set(want)))
    assert (0x017F, ord("s")) in t.folds                         # LATIN SMALL LETTER LONG S: the one partner beyond ASCII


def test_general_categories_equal_the_engine(table_and_probe):
    _, t, p = table_and_probe
    want = np.zeros(N_CP, dtype=np.uint8)                       # Cn: what no other category claims
    for code, name in enumerate(GC_NAMES):
        if name in ("Cn", "Cs"):
            continue
        m = p.members(r"\p{%s}+" % name)
        assert not want[m].any(), name
        want[m] = code
    want[0xD800:0xE000] = GC_NAMES.index("Cs")
    d = np.nonzero(t.gc != want)[0]
    assert not len(d), (f"{len(d)} code points have another general category in the engine, first U+{int(d[0]):04X}: "
                        f"table {GC_NAMES[t.gc[d[0]]]}, engine {GC_NAMES[want[d[0]]]}")


def test_scripts_equal_the_engine(table_and_probe):
    _, t, p = table_and_probe
    assert len(t.scripts) > 150
    for name, ranges in t.scripts:
        have = np.zeros(N_CP, dtype=bool)
        for a, b in ranges:
            assert a <= b
            have[a:b + 1] = True
        have[0xD800:0xE000] = False                             # (a range may run across the surrogates: they never occur)
        _differ(r"\p{%s}" % name, have, p.members(r"\p{%s}+" % name))
    # ... and a script name the generator knows but the table lacks is one the engine does not know, or one without a member
    spec = importlib.util.spec_from_file_location("gen_unicode_tables", os.path.join(ROOT, "tools", "gen_unicode_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        spec.loader.exec_module(gen)                            # (defines; main() is not run, nothing is written)
    for name in sorted(set(gen.SCRIPT_NAMES) - {n for n, _ in t.scripts}):
        m = p.knows(r"\p{%s}+" % name)
        assert m is None or not m.any(), name


# ------------------------------------------------------------------------------------------------
# the generator's own promises
# ------------------------------------------------------------------------------------------------
def test_sweeps_cover_what_they_promise():
    """full_sweep() and reduced_sweep() assert their coverage before they return (four alignments, first and last position, the
    thinned range uniform, every scalar value); here the same from the packed bytes alone, for a sample, and the map back"""
    for fn, _ in TABLES:
        assert cpsweep.uniform_range(fn, cpsweep.THIN_RANGE) == (CLASS_NAMES.index("P"), GC_NAMES.index("Cn"))
    with pytest.raises(AssertionError, match="not uniform"):
        cpsweep.uniform_range("unicode_classes.bin", (0x30000, 0xDFFFF))        # (U+30000..U+3134A are Lo)
    full, red = cpsweep.full_sweep(), cpsweep.reduced_sweep()
    text, off = full.packed()
    assert int(off[-1]) == full.n_bytes == len(text) and len(off) == len(full.docs) + 1
    blob = text.tobytes()
    starts = set(off[:-1].tolist())
    ends = set(off[1:].tolist())
    for cp in (0x41, 0x7F, 0x80, 0x17F, 0x7FF, 0x800, 0x4E00, 0x9FFF, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x2FA1D, 0x3134A, 0x3FFFF, 0xE0001, 0x10FFFF):
        needle, at, seen = chr(cp).encode("utf-8"), -1, []
        while True:
            at = blob.find(needle, at + 1)
            if at < 0:
                break
            seen.append(at)
        assert {a & 3 for a in seen} == {0, 1, 2, 3}, hex(cp)
        assert any(a in starts for a in seen) and any(a + len(needle) in ends for a in seen), hex(cp)
    assert blob.count(chr(0x40000).encode()) == 2 and blob.count(chr(0xDFFFF).encode()) == 2      # thinned: 'X ' and alone
    d = 40000                                                   # (a document of a context, not of one character)
    cp, ctx = full.locate(d, len(full.docs[d]) // 2)
    assert chr(cp).encode("utf-8") in full.docs[d] and ctx in cpsweep.FULL_CONTEXTS and f"U+{cp:04X} in context {ctx!r}" in full.describe(d, len(full.docs[d]) // 2)
    assert red.n_bytes < full.n_bytes // 3 and b"".join(red.docs).count(b"\n") == 1112064 + 2      # (one per piece, and U+000A itself twice)
    print(f"full sweep {full.n_bytes} bytes in {len(full.docs)} documents, reduced sweep {red.n_bytes} bytes in {len(red.docs)} documents")


# ------------------------------------------------------------------------------------------------
# (b) the C oracle equals PCRE2 on the full sweep
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_vs_pcre2():
    """every document of the full sweep split by PCRE2's find_iter and by the C oracle, all three patterns, in a pool of processes
    (started afresh, not forked: the suite's process may hold a GPU)"""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    from oracle import pyoracle as O
    from oracle import coracle
    if not O.pcre2_available():
        pytest.skip("libpcre2-8 not present")
    coracle.build()
    full = cpsweep.full_sweep()
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    docs = full.docs
    # tasks of about equal BYTES (the documents of one character are a million of the 1.2 million)
    sizes = np.cumsum([len(d) for d in docs])
    cuts = np.searchsorted(sizes, np.linspace(0, sizes[-1], workers * 4 + 1)[1:-1]).tolist()
    edges = [0] + cuts + [len(docs)]
    tasks = [(a, docs[a:b], PATTERNS) for a, b in zip(edges[:-1], edges[1:]) if b > a]
    t0 = time.perf_counter()
    with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as pool:
        results = list(pool.map(cpsweep.split_check_worker, tasks))
    wall = time.perf_counter() - t0
    print(f"C oracle against PCRE2: {full.n_bytes} bytes, {len(docs)} documents, 3 patterns, {workers} processes: {wall:.1f} s wall; "
          + "; ".join(f"{n}: PCRE2 {sum(r[n][1] for r in results):.1f} s, oracle {sum(r[n][2] for r in results):.1f} s of CPU" for n in PATTERNS))
    return full, results


@pytest.mark.parametrize("name", PATTERNS)
def test_c_oracle_splits_the_full_sweep_as_pcre2_does(oracle_vs_pcre2, name):
    from oracle import pyoracle as O
    full, results = oracle_vs_pcre2
    bad = sorted(r[name][0] for r in results if r[name][0] >= 0)
    if bad:
        d = bad[0]
        doc = full.docs[d]
        want = [a for a, _ in O.split_pcre2(O.PRETRAINED[name][1], doc)]
        from oracle.coracle import COracle
        got = COracle(name).split_bytes(doc)
        k = next(i for i in range(max(len(got), len(want))) if i >= len(got) or i >= len(want) or got[i] != want[i])
        at = min(got[k] if k < len(got) else len(doc) - 1, want[k] if k < len(want) else len(doc) - 1)
        raise AssertionError(f"{name}: {len(bad)} task(s) differ; first at {full.describe(d, at)}: oracle {got[k:k + 4]}, PCRE2 {want[k:k + 4]}")


# ------------------------------------------------------------------------------------------------
# (c) the host compile of the scanner headers on the reduced sweep
# ------------------------------------------------------------------------------------------------
def _first_split_difference(got, want):
    """(index of the first start that differs, the byte it lies at)"""
    k = next(k for k in range(max(len(got), len(want))) if k >= len(got) or k >= len(want) or got[k] != want[k])
    return k, min(got[k] if k < len(got) else 1 << 30, want[k] if k < len(want) else 1 << 30)


@pytest.mark.parametrize("name", PATTERNS)
def test_hostsim_splits_the_reduced_sweep_as_the_oracle_does(coracle, name):
    """spl_scan_words.h / spl_scan_starts.h / spl_scan_masks.h compiled for the host, tiled like the kernel in both geometries of the
    tile-owned mode and at the smallest mask window (hs_split_* keep no state in the handle: groups of documents run on threads)"""
    from concurrent.futures import ThreadPoolExecutor
    from hostsim import HostSim
    h, c = HostSim(name), coracle(name)
    red = cpsweep.reduced_sweep()
    t0 = time.perf_counter()
    ref = [c.split_bytes(d) for d in red.docs]
    group = 16

    def run(i):
        docs, want = red.docs[i:i + group], ref[i:i + group]
        for tb, rh in ((800, 192), (864, 128)):
            got, _ = h.split_starts(docs, tb, rh, 16)
            for j in range(len(docs)):
                if got[j] != want[j]:
                    k, at = _first_split_difference(got[j], want[j])
                    return f"split_starts({tb}, {rh}): {red.describe(i + j, at)}: {got[j][k:k + 4]} instead of {want[j][k:k + 4]}"
        for j, d in enumerate(docs):
            got = h.split_masks(d, 64, 32)
            if got != want[j]:
                k, at = _first_split_difference(got, want[j])
                return f"split_masks(64, 32): {red.describe(i + j, at)}: {got[k:k + 4]} instead of {want[j][k:k + 4]}"
        return None
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        bad = [r for r in pool.map(run, range(0, len(red.docs), group)) if r]
    assert not bad, f"{name}: {len(bad)} group(s) of documents differ, first {bad[0]}"
    print(f"{name}: HostSim on {red.n_bytes} bytes, two tile geometries and the mask scanner: {time.perf_counter() - t0:.1f} s")
