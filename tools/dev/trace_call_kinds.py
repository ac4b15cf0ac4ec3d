"""One call each of the four kinds of device call (latency path, pinned one-chunk host batch, device batch, pipeline of 64 KB chunks),
for a kernel trace (profiles/launch_request.txt):
    rocprofv3 --kernel-trace --output-format csv -d OUT -o NAME -- python tools/dev/trace_call_kinds.py ROOT
ROOT: the tree whose library runs (so that two commits can be traced by one script)."""
import ctypes
import os
import sys

ROOT = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from splintr_amd import Tokenizer, corpus, _ffi  # noqa: E402
from splintr_amd.device import DeviceBatch, encode_device  # noqa: E402

L = _ffi.lib()
dev = torch.device("cuda", 0)


def packed(docs):
    bs = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return b"".join(bs), off


docs = corpus.c2(400, seed=7)
t = Tokenizer.from_pretrained("cl100k_base")
# 1: latency path
n1 = len(t.encode(docs[0][:100]))
torch.cuda.synchronize()
# 2: pinned one-chunk host batch, ~64 KB
blob, off = packed(docs[:64])
p = L.spl_host_alloc(len(blob) + 64)
ctypes.memmove(p, blob, len(blob))
ids2, _ = t._encode_packed(p, off.ctypes.data, 64, 0)
torch.cuda.synchronize()
# 3: device batch, ~64 KB
b = DeviceBatch(docs[64:128], dev)
encode_device(t, b)
torch.cuda.synchronize()
n3 = int(b.out_off[-1].item())
# 4: pipeline of 64 KB chunks over ~200 KB, pageable
assert L.spl_set_option(t.handle, b"chunk_bytes", 1 << 16) == 0
blob4, off4 = packed(docs[128:328])
ids4, _ = t.encode_packed(blob4, off4)
torch.cuda.synchronize()
L.spl_host_free(p)
print("trace_call_kinds", ROOT, "bytes", 100, len(blob), b.n_bytes, len(blob4), "tokens", n1, len(ids2), n3, len(ids4))
