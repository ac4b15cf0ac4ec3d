"""Counter-pass driver (a -DSPL_DEBUG_STAMPS build via SPL_LIB_PATH): the bench batch with the memo warm (or off), then k_pretok cut off
after each phase.  Launch order: WARM full launches, 20 full launches (stop 0), then stops 7, 6, ... 1 with 20 launches each -- never a
full launch behind a cut one (a cut fused launch publishes no counts).  tools/dev/pmc_phase_sum.py groups the dispatches by this order."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from splintr_amd import Tokenizer, corpus, _ffi
from splintr_amd.device import DeviceBatch, encode_device, reserve
L = _ffi.lib(); L.spl_memo_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
memo = int(sys.argv[1])
WARM, N = 30, 20
tok = Tokenizer.from_pretrained("cl100k_base")
texts = corpus.c2(1000)
if os.environ.get("SPL_ASCII_CONTROL") == "1":        # (the accented letters as their base letters: tools/dev/two_byte_ceiling.py)
    from two_byte_ceiling import ascii_control
    texts = ascii_control(texts)
batch = DeviceBatch(texts, torch.device("cuda", 0))
reserve(tok, batch.n_bytes, batch.n_docs)
assert L.spl_set_option(tok.handle, b"memo", memo) == 0
st = (ctypes.c_uint64 * 16)()
for _ in range(WARM):
    encode_device(tok, batch); torch.cuda.synchronize()
ms = (ctypes.c_uint64 * 4)()
L.spl_memo_stats(tok.handle, ms)
print("memo stats after warm-up:", list(ms), flush=True)
for stop in (0, 7, 6, 5, 4, 3, 2, 1):
    L.spl_debug_phases(tok.handle, stop << 4, st)
    for _ in range(N):
        encode_device(tok, batch)
    torch.cuda.synchronize()
print("done", flush=True)
