"""GPU test (-m gpu): no option of one device call outlives the call.  What a call wants -- the two-launch form for text read in place,
the host address its offsets also go to, the completion word of the latency path -- travels in its request (csrc/spl_launch.h LaunchReq),
not in the context, so the calls of one handle can follow each other in any order, behind a refused call too, and each runs in its own
form and writes into its own buffers only.  One handle (cl100k_base), per-kernel profiling on: every device call asserts the form it ran
in from the launch counts, as test_gpu_fused does (slot 8, k_tile_out, does not move for a fused launch), and every result is the oracle's.
"""
import ctypes
import os
import random

import numpy as np
import pytest

from test_gpu_fused import NAME, POISON, _dev, _encode, _launches, _lib, _opt, _profile, _same, _tiles, _want
from test_host_regex import GPT2_PATTERN

pytestmark = pytest.mark.gpu

SPL_EINVAL = -1
OFF_POISON = 0xA5A5A5A5A5A5A5A5


def _packed(docs):
    bs = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return b"".join(bs), off


class _PinnedResult:
    """spl_encode_batch from pinned text, its result kept alive: views of the pinned ids and offsets the kernels wrote."""

    def __init__(self, t, docs):
        L = _lib()
        blob, self.host_off = _packed(docs)
        self.text = L.spl_host_alloc(len(blob) + 64)
        assert self.text
        ctypes.memmove(self.text, blob, len(blob))
        self.res = ctypes.c_void_p()
        self.call = lambda: L.spl_encode_batch(t.handle, self.text, self.host_off.ctypes.data, len(docs), 0, ctypes.byref(self.res))
        self.n_docs = len(docs)

    def views(self):
        L = _lib()
        n = L.spl_result_n_tokens(self.res)
        return (np.ctypeslib.as_array(L.spl_result_tokens(self.res), shape=(n,)),
                np.ctypeslib.as_array(L.spl_result_offsets(self.res), shape=(self.n_docs + 1,)))

    def free(self):
        _lib().spl_result_free(self.res)
        _lib().spl_host_free(self.text)


def test_no_option_of_a_call_outlives_it(coracle):
    import torch
    from splintr_amd import Tokenizer
    from splintr_amd.device import DeviceBatch
    L = _lib()
    rng = random.Random(77)
    dev = _dev()
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = Tokenizer.from_pretrained(NAME)
    _profile(t, True)

    short = "".join(_tiles("c2", 61, 1, rng, short=700))                 # 100 bytes: the latency path
    want_short = _want(coracle, [short])[0].tolist()
    d80, d80b, d3 = _tiles("c2", 61, 80, rng), _tiles("c3", 62, 80, rng), _tiles("c2_wide", 63, 3, rng)
    pinned_docs = _tiles("c3", 62, 80, rng)                              # ~64 KB, one chunk
    piped_docs = _tiles("c2", 64, 250, rng)                              # ~200 KB: chunks of 64 KB
    b80, b80b, b3 = DeviceBatch(d80, dev), DeviceBatch(d80b, dev), DeviceBatch(d3, dev)
    w80, w80b, w3 = _want(coracle, d80), _want(coracle, d80b), _want(coracle, d3)

    def latency_call(what):                                             # 1: arms the completion word, offsets written to the host
        before = L.spl_small_path_calls(t.handle)
        assert t.encode(short) == want_short, what
        assert L.spl_small_path_calls(t.handle) - before == 1, what

    kept = None

    def device_call(b, want, what):                                     # 3: fused, and nothing of an earlier call's addresses is written
        _same(_encode(t, b, "fused"), want, what)
        torch.cuda.synchronize()
        ids, off = kept
        assert (off == OFF_POISON).all() and (ids == POISON).all(), f"{what}: an earlier call's pinned result was written to"

    latency_call("step 1")
    # 2: a one-chunk batch from pinned text -- read in place, which takes the two-launch form (slot 8 counts it), ids and offsets written
    #    into the pinned result by k_tile_out
    pr = _PinnedResult(t, pinned_docs)
    try:
        rcs = []
        n_pretok, n_out = _launches(t, lambda: rcs.append(pr.call()))
        assert rcs == [0] and (n_pretok, n_out) == (1, 1), (rcs, n_pretok, n_out)
        ids, off = pr.views()
        _same((ids.copy(), off.copy()), _want(coracle, pinned_docs), "step 2: pinned one-chunk batch")
        ids[:] = POISON
        off[:] = OFF_POISON
        kept = (ids, off)
        device_call(b80, w80, "step 3: 80 tiles behind the pinned batch")
        # 4: a pipeline of several chunks from pageable text: consecutive chunks' kernels alternate between the context and its twin, each
        #    chunk's offsets go to the lane's pinned staging.  (The pipeline takes no twin while per-kernel profiling is on: off for this step.)
        _profile(t, False)
        _opt(t, "chunk_bytes", 1 << 16)
        try:
            blob, hoff = _packed(piped_docs)
            assert len(blob) > 3 * (1 << 16)
            _same(t.encode_packed(blob, hoff), _want(coracle, piped_docs), "step 4: pipeline")
        finally:
            _opt(t, "chunk_bytes", 5 << 20)
            _profile(t, True)
        latency_call("step 5")
        device_call(b80b, w80b, "step 5: 80 tiles behind the pipeline and the latency path")

        # 6: calls refused on the host -- nothing launched -- and behind them two fused launches of different tile counts
        n = _launches(t, lambda: rcs.append(L.spl_encode_batch_device(
            t.handle, b80.text.data_ptr() + 1, b80.n_bytes - 1, b80.doc_off.data_ptr(), b80.n_docs, 1, b80.ids.data_ptr(), b80.ids.numel(),
            b80.out_off.data_ptr(), stream)))
        assert rcs[-1] == SPL_EINVAL and n == (0, 0), (rcs, n)
        with open(os.path.join(os.path.dirname(__file__), "..", "splintr_amd", "data", NAME + ".splv"), "rb") as f:
            tc = Tokenizer.from_bytes(f.read(), GPT2_PATTERN)
        assert tc.has_custom_pattern
        tiny = DeviceBatch(["x"], dev)
        # (a COUNT beyond the device splitter's 256 MB, refused before the text is looked at)
        rc = L.spl_encode_batch_device(tc.handle, tiny.text.data_ptr(), (256 << 20) + 1, tiny.doc_off.data_ptr(), 1, 0, tiny.ids.data_ptr(),
                                       tiny.ids.numel(), tiny.out_off.data_ptr(), stream)
        assert rc == SPL_EINVAL, rc
        device_call(b80, w80, "step 6: 80 tiles behind the refused calls")
        device_call(b3, w3, "step 6: 3 tiles")
    finally:
        torch.cuda.synchronize()
        pr.free()
        _profile(t, False)
