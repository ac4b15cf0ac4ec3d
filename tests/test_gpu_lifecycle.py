"""GPU tests (-m gpu) of what a handle OWNS over its life: every buffer of a context belongs to a member that frees it
(splintr_amd/csrc/spl_host_res.h), and every path that frees and re-allocates one -- the workspace growing, the memo dropped and
rebuilt, the staging slots, the twin, specials and decode tables uploaded again, new contexts, the handle destroyed under a live
result -- runs here on ONE handle, each result against the C oracle.  Then the same for a custom-pattern handle (exact ids against the
host splitter's handle, which tests/test_host_regex.py pins to PCRE2), and a loop that shows destroyed handles give their memory back."""
import ctypes
import gc

import numpy as np
import pytest

from test_gpu_device_split import _blob
from test_gpu_parity import oracle_csr
from test_host_regex import GPT2_PATTERN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(coracle):
    """The 6 MB batch (1 500 documents of ~4 KB) and its CSR from the oracle, computed once.  A batch of its first k documents has the
    first k + 1 offsets and the ids in front of offset k."""
    from splintr_amd import corpus
    docs = corpus.c3(1500, seed=11)
    ids, off = oracle_csr(coracle("cl100k_base"), docs)
    return docs, ids, off


def _prefix(ref, k):
    docs, ids, off = ref
    return docs[:k], ids[:int(off[k])], off[:k + 1]


def _same(got, want_ids, want_off, what):
    assert np.array_equal(got[1], want_off), what
    assert np.array_equal(got[0], want_ids), what


def _opt(t, **opts):
    from splintr_amd import _ffi
    for k, v in opts.items():
        assert _ffi.lib().spl_set_option(t.handle, k.encode(), int(v)) == 0, _ffi.last_error()


N200K, N3M = 50, 750          # documents of the 200 KB and of the 3 MB batch


def test_every_reallocation_path_in_one_handle(coracle, ref):
    from oracle.coracle import COracle, lib as orc_lib
    from splintr_amd import Tokenizer, _ffi
    L = _ffi.lib()
    docs, ids6, off6 = ref
    d200, ids200, off200 = _prefix(ref, N200K)
    t = Tokenizer.from_pretrained("cl100k_base")
    # 3 KB: the latency path (its pinned block, the workspace's first size)
    tiny = [d[:180] for d in docs[:16]]
    while sum(len(x.encode()) for x in tiny) > 3072:
        tiny.pop()
    assert len(tiny) >= 8
    before = L.spl_small_path_calls(t.handle)
    _same(t.encode_batch_csr(tiny), *oracle_csr(coracle("cl100k_base"), tiny), "3 KB")
    assert L.spl_small_path_calls(t.handle) == before + 1
    # 200 KB: one chunk, one fused launch; the workspace grows, the memo is built
    _same(t.encode_batch_csr(d200), ids200, off200, "200 KB")
    # 6 MB in chunks of 1 MB: staging slots, the lane's ids, the twin and its workspace
    _opt(t, chunk_bytes=1 << 20)
    _same(t.encode_batch_csr(docs), ids6, off6, "6 MB pipelined")
    # the memo dropped and rebuilt three times (in the context and in its twin)
    for opts in ({"memo_bits": 8}, {"memo_long_bits": 0}, {"memo_bits": 20, "memo_long_bits": 16}):
        _opt(t, **opts)
        _same(t.encode_batch_csr(d200), ids200, off200, f"200 KB after {opts}")
        _same(t.encode_batch_csr(d200), ids200, off200, f"200 KB after {opts}, memo warm")
    _same(t.encode_batch_csr(docs), ids6, off6, "6 MB pipelined, memos rebuilt")
    # a special token added after the tables were used: specials and decode tables go up again
    lit, lit_id = "<|lifecycle|>", 100400
    assert L.spl_add_special(t.handle, lit.encode(), len(lit.encode()), lit_id) == 0, _ffi.last_error()
    orc = COracle("cl100k_base")                                    # (a private oracle: the shared one keeps its special tokens)
    orc_lib().orc_add_special(orc._h, lit.encode(), len(lit.encode()), lit_id)
    sp_docs = [d + lit + "<|endoftext|>" for d in d200[:20]] + [lit, "", lit + lit]
    want_ids, want_off = oracle_csr(orc, sp_docs, True)
    assert lit_id in want_ids
    got = t.encode_batch_with_special(sp_docs)
    assert got == [want_ids[int(want_off[i]):int(want_off[i + 1])].tolist() for i in range(len(sp_docs))]
    assert t._decode_batch_bytes(got) == [d.encode() for d in sp_docs]
    # a larger one-chunk batch than any before: the workspace grows again
    _opt(t, chunk_bytes=5 << 20)
    _same(t.encode_batch_csr(docs[:N3M]), ids6[:int(off6[N3M])], off6[:N3M + 1], "3 MB, one chunk")
    # new contexts (the old one and its twin are destroyed), the 6 MB batch across the two
    _opt(t, chunk_bytes=1 << 20)
    t.set_devices([0, 0])
    _same(t.encode_batch_csr(docs), ids6, off6, "6 MB over two contexts")
    # a result outlives its handle: its pinned buffers belong to the pool the two share
    bs = [x.encode() for x in d200]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    res = ctypes.c_void_p()
    assert L.spl_encode_batch(t.handle, b"".join(bs), off.ctypes.data, len(bs), 0, ctypes.byref(res)) == 0, _ffi.last_error()
    L.spl_destroy(t.handle)
    t._h = None
    try:
        nt = L.spl_result_n_tokens(res)
        assert nt == len(ids200)
        assert np.array_equal(np.ctypeslib.as_array(L.spl_result_tokens(res), shape=(nt,)), ids200)
        assert np.array_equal(np.ctypeslib.as_array(L.spl_result_offsets(res), shape=(len(bs) + 1,)), off200)
    finally:
        L.spl_result_free(res)


def _encode_device(t, texts):
    import torch
    from splintr_amd import _ffi
    from splintr_amd.device import DeviceBatch
    db = DeviceBatch(texts, torch.device("cuda", 0))
    db.ids.fill_(-1)
    rc = _ffi.lib().spl_encode_batch_device(t.handle, db.text.data_ptr(), db.n_bytes, db.doc_off.data_ptr(), db.n_docs, 0, db.ids.data_ptr(),
                                            db.ids.numel(), db.out_off.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _ffi.last_error()
    torch.cuda.synchronize()
    off = db.out_off.cpu().numpy().astype(np.uint64)
    return db.ids[:int(off[-1])].cpu().numpy().view(np.uint32), off


def test_custom_pattern_handle_grows_and_patches(ref):
    """GPT-2's pattern on cl100k's vocabulary, text in device memory: the splitter's bitmaps and workspace grow with the batch; a run
    of '=' longer than the device matcher's reach sends ITS document to the host, whose patch buffer is allocated by the first such
    batch and grown by the second (three documents, each eight times the first one's size)."""
    from splintr_amd import Tokenizer, _ffi
    L = _ffi.lib()
    docs = ref[0]
    t = Tokenizer.from_bytes(_blob("cl100k_base"), GPT2_PATTERN)
    h = Tokenizer.from_bytes(_blob("cl100k_base"), GPT2_PATTERN)
    assert L.spl_set_option(h.handle, b"device_split", 0) == 0
    run = "=" * 2048

    def step(texts, fallbacks, what):
        before = L.spl_device_split_fallbacks(t.handle)
        _same(_encode_device(t, texts), *h.encode_batch_csr(texts), what)
        assert L.spl_device_split_fallbacks(t.handle) - before == fallbacks, what
    step(docs[:16], 0, "64 KB")
    step(docs[:75], 0, "300 KB")
    one = docs[:16]
    one[5] = one[5][:300] + run + one[5][300:1500]
    step(one, 1, "one document with a 2 KB run")
    three = docs[:16]
    for i in (2, 7, 11):
        three[i] = "".join(docs[20 + i:28 + i])[:30000] + run + " tail"
    step(three, 3, "three larger documents with a 2 KB run")
    step(docs[:16], 0, "64 KB again")


def test_handles_do_not_leak_device_memory(ref):
    """Eight times: a handle, the 200 KB batch, the 6 MB batch through the pipeline (slots, twin), one decode, the handle destroyed; free
    device memory read after each cycle (the first two absorb what the runtime allocates once).  Measured on an MI355X, cycle 2 to
    cycle 8: 0 bytes lost with the hand-written frees of the parent commit, 0 bytes with the owners.  The bound is the parent's drift
    plus the smallest workspace buffer the loop allocates -- the tile-control words of the 200 KB batch, (16 + 4 * (271 / 64 + 2) + 2) * 4 = 168 bytes --
    so that one workspace buffer lost per cycle (six in all) fails."""
    import torch
    from splintr_amd import Tokenizer
    docs, ids6, off6 = ref
    d200, ids200, off200 = _prefix(ref, N200K)
    lists = [ids200[int(off200[i]):int(off200[i + 1])].tolist() for i in range(N200K)]
    free = []
    for _ in range(8):
        t = Tokenizer.from_pretrained("cl100k_base")
        _same(t.encode_batch_csr(d200), ids200, off200, "200 KB")
        _same(t.encode_batch_csr(docs), ids6, off6, "6 MB pipelined")
        assert t._decode_batch_bytes(lists) == [d.encode() for d in d200]
        del t
        gc.collect()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    drift = free[1] - free[7]
    print(f"free device memory after each cycle: {free}; lost from cycle 2 to cycle 8: {drift} bytes")
    assert drift <= 0 + 168, free
