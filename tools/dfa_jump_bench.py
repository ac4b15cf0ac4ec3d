"""Jump-forward for the regex guide on the GPU -> profiles/dfa_jump.txt.

  (i) the jump index       spl_dfa_jump_index_device for the date, JSON-object and (a|b)*a(a|b){10} patterns on cl100k_base and o200k_base,
                           beside spl_dfa_index_device on the same table.  The call synchronises once by itself, so it is timed on the
                           host around the call and a synchronisation (the plain index likewise, for the comparison).  The split --
                           force + runs | the compaction and its read-back | the encode | the scatter -- comes from the "jump_phase"
                           option, which makes the call return behind a phase: medians of the truncated calls, differences of those.
  (s) the step             spl_dfa_jump_device against spl_dfa_step_device at B = 256 and 4096, K = 1, device events around bursts of
                           STEPS calls into preallocated outputs, state carried:
                             (s0) spl_dfa_step_device                              -- this build's; the PARENT's is tools/dfa_bench.py's (c) run
                                                                                      from the parent's tree in turn with this file
                             (a)  spl_dfa_jump_device with a jump index of zeros   -- the same work and one byte load a sequence
                             (b)  spl_dfa_jump_device, the JSON pattern, every sequence of every call in a FORCED state (the state is not
                                  carried: each call starts from the pattern's start state and emits its run)
  (d) the draws            the end-to-end loop of tests/test_gpu_dfa_jump.py: 256 sequences of the JSON pattern, a uniform sampler, draws
                           (forward passes of a model) with and without jump

No ratio is a bar here: nothing of this had been measured."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from choice_bench import vocabulary  # noqa: E402
from dfa_bench import INDEX_PATTERNS  # noqa: E402
from stop_bench import event_bursts  # noqa: E402
from stream_bench import STEPS, stat  # noqa: E402
from splintr_amd import Tokenizer, _ffi, dfa  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

JSON = r'\{"name": "[a-z]+", "age": [0-9]{1,3}\}'
PHASES = ["force + runs", "compaction + read-back", "encode", "scatter"]


def wall(fn, rounds, warm=2):
    """[ms, one per call]: the call and a synchronisation behind it, on the host's clock"""
    out = []
    for r in range(warm + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def uniform(mask, gen, only):
    B, nw = mask.shape
    shifts = torch.arange(32, device=mask.device, dtype=torch.int32)
    bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, nw * 32).to(torch.float32)
    narrowed = bits * only
    bits = torch.where(narrowed.sum(1, keepdim=True) > 0, narrowed, bits)     # (a row the restriction would empty keeps its whole mask)
    return torch.multinomial(bits, 1, generator=gen).flatten()


def draws(tok, special, by_id, jump, B=256, seed=5, leave_after=3, max_steps=48):
    """The loop of tests/test_gpu_dfa_jump.py: begin(), then jump() (or step()) and a uniform draw from the mask until every sequence is
    done; once a sequence has drawn leave_after ids in states that are not forced, its draw is uniform over the allowed ids without a
    lower-case letter (the name has no upper bound).  -> (draws over the batch, END included; the texts)"""
    import re
    d = dfa.compile_regex(JSON)
    S = d.n_states
    forced_state = [(not d.accept[q]) and int((d.trans[q] < S).sum()) == 1 for q in range(S)]
    guide = tok.regex_guide(B, d, end_ids=[special], jump=jump)
    dev = guide.mask.device
    lower = re.compile(rb"[a-z]")
    no_letters = torch.zeros(guide.n_words * 32, dtype=torch.float32, device=dev)
    no_letters[torch.tensor([i for i, b in by_id.items() if not lower.search(b)] + [special], device=dev)] = 1.0
    gen = torch.Generator(device=dev).manual_seed(seed)
    texts, free_draws, n = [b""] * B, [0] * B, 0

    def take(forced, flen):
        for b, (row, m) in enumerate(zip(forced.cpu().tolist(), flen.cpu().tolist())):
            texts[b] += b"".join(by_id[t] for t in row[:m])

    guide.begin()
    if jump:
        take(*guide.jump())
    for step in range(max_steps):
        live = guide.live.cpu().numpy().astype(bool)
        if not live.any():
            break
        leave = torch.tensor([[1.0 if k >= leave_after else 0.0] for k in free_draws], device=dev)
        pick = uniform(guide.mask, gen, leave * no_letters + (1.0 - leave))
        q = guide.q.cpu().tolist()
        for b, t in enumerate(pick.cpu().tolist()):
            if live[b]:
                n += 1
                if t != special:
                    free_draws[b] += not forced_state[q[b]]
                    texts[b] += by_id[t]
        lens = guide.live.to(torch.int32)
        if jump:
            take(*guide.jump(pick, lens))
        else:
            guide.step(pick, lens)
    assert guide.done.all().item() and all(re.fullmatch(JSON.encode(), t) for t in texts)
    return n, texts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--index-rounds", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("dfa_jump_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs, unit="us", scale=1e3):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<78} median {med * scale:10.2f} {unit}   min {lo * scale:10.2f}  max {hi * scale:10.2f}  spread {spread * scale:9.2f} {unit}   [{len(xs)}]")
        return med, spread

    emit(f"dfa_jump_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; step bursts of {STEPS} calls; per CALL of the batch")
    summary = []
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        toks, special = vocabulary(tok)
        by_id = dict(toks)
        nw = dv.dfa_n_words(tok)
        dv.dfa_reserve(tok)
        emit()
        emit(f"== {name}: V = {tok.vocab_size}, n_words = {nw}, END id {special}")
        emit("  (i) the jump index beside the index: host clock around the call and a synchronisation; the phases by \"jump_phase\"")
        for label, pat in INDEX_PATTERNS.items():
            d = dfa.compile_regex(pat)
            S = d.n_states
            table = dv.dfa_table(d, dev)
            out_i = torch.empty(_ffi.SPL_DFA_INDEX_BYTES(S, nw), dtype=torch.uint8, device=dev)
            out_j = torch.empty(_ffi.SPL_DFA_JUMP_INDEX_BYTES(S), dtype=torch.uint8, device=dev)
            emit(f"  -- {label}: {S} states, jump index {out_j.numel() / 1e3:.1f} KB, index {out_i.numel() / 1e6:.1f} MB")
            mi, _ = line("spl_dfa_index_device", wall(lambda: dv.dfa_index_device(tok, table, S, n_words=nw, out=out_i), args.index_rounds), "us")
            cum = []
            for phase in (1, 2, 3, 0):
                assert _ffi.lib().spl_set_option(tok.handle, b"jump_phase", phase) == 0
                cum.append(stat(wall(lambda: dv.dfa_jump_index_device(tok, table, S, out=out_j), args.index_rounds))[0])
            assert _ffi.lib().spl_set_option(tok.handle, b"jump_phase", 0) == 0
            mj, _ = line("spl_dfa_jump_index_device, whole", wall(lambda: dv.dfa_jump_index_device(tok, table, S, out=out_j), args.index_rounds), "us")
            parts = [cum[0], cum[1] - cum[0], cum[2] - cum[1], cum[3] - cum[2]]
            emit("     split (medians of truncated calls, differences): " + "; ".join(f"{p} {x * 1e3:.1f} us" for p, x in zip(PHASES, parts)))
            ids, n_ids, run_len, run = dv.dfa_jump_index_views(out_j, S)
            emit(f"     -> {int((run_len > 0).sum().item())} forced states, {int(run_len.sum().item())} run bytes, {int(n_ids.sum().item())} ids; "
                 f"the longest run {int(run_len.max().item())} bytes; jump index / index = {mj / mi:.2f}")
            summary.append(f"jump index {name} {label}: {S} states {mj * 1e3:.0f} us (index {mi * 1e3:.0f} us): " +
                           " | ".join(f"{x * 1e3:.0f}" for x in parts) + " us")
        # the steps
        d = dfa.compile_regex(JSON)
        S = d.n_states
        emit(f"  (s) the step: {JSON!r}: {S} states")
        for B in map(int, args.sizes.split(",")):
            guide = dv.RegexGuide(tok, B, d, end_ids=[special], jump=True)
            guide.begin()
            state0 = guide.state.clone()
            # a script of draws that keeps every sequence constrained: the token "a" (a letter of the name, for ever)
            guide.jump()
            state1 = guide.state.clone()
            script = [torch.full((B,), tok.encode("a")[0], dtype=torch.int64, device=dev) for k in range(STEPS)]
            for ids in script:
                guide.step(ids)
            assert guide.live.all().item() and not guide.broken.any().item()
            zero = torch.zeros_like(guide.jump_index)
            mask = torch.empty_like(guide.mask)
            cur = state1.clone()
            live = torch.empty(B, dtype=torch.uint8, device=dev)
            forced = torch.zeros((B, 16), dtype=torch.int32, device=dev)
            flen = torch.zeros(B, dtype=torch.int32, device=dev)
            common = dict(end_ids=[special], n_states=S, mask=mask, live=live)

            def s0(k):
                dv.dfa_step_device(tok, script[k], None, cur, guide.table, guide.index, state_out=cur, **common)

            def sa(k):
                dv.dfa_jump_device(tok, script[k], None, cur, guide.table, guide.index, zero, state_out=cur, forced_ids=forced, forced_len=flen, **common)

            out_b = torch.empty_like(state0)

            def sb(k):
                dv.dfa_jump_device(tok, None, None, state0, guide.table, guide.index, guide.jump_index, state_out=out_b, forced_ids=forced, forced_len=flen,
                                   **common)

            def sb0(k):
                dv.dfa_step_device(tok, None, None, state0, guide.table, guide.index, state_out=out_b, **common)
            # the same four through the C ABI with the structs built once: a burst is then bound by the device, not by the Python wrapper
            L, h, stream = _ffi.lib(), tok.handle, torch.cuda.current_stream(dev).cuda_stream
            ref = ctypes.byref
            si = _ffi.SplDfaIn(B, 1, script[0].data_ptr(), None, cur.data_ptr(), guide.table.data_ptr(), guide.index.data_ptr(), S)
            sib = _ffi.SplDfaIn(B, 0, None, None, state0.data_ptr(), guide.table.data_ptr(), guide.index.data_ptr(), S)
            o = _ffi.SplDfaOpts(_ffi.SPL_DFA_I64, nw, [special])
            so = _ffi.SplDfaOut(cur.data_ptr(), mask.data_ptr(), live.data_ptr())
            sob = _ffi.SplDfaOut(out_b.data_ptr(), mask.data_ptr(), live.data_ptr())
            jz = _ffi.SplDfaJumpOut(16, zero.data_ptr(), forced.data_ptr(), flen.data_ptr())
            jb = _ffi.SplDfaJumpOut(16, guide.jump_index.data_ptr(), forced.data_ptr(), flen.data_ptr())

            def ok(rc):
                assert rc == 0, _ffi.last_error()
            fresh = lambda: cur.copy_(state1)
            none = lambda: None
            e = event_bursts({"s0": (fresh, s0), "a": (fresh, sa), "b0": (none, sb0), "b": (none, sb),
                              "c_s0": (fresh, lambda k: ok(L.spl_dfa_step_device(h, ref(si), ref(o), ref(so), stream))),
                              "c_a": (fresh, lambda k: ok(L.spl_dfa_jump_device(h, ref(si), ref(o), ref(so), ref(jz), stream))),
                              "c_b0": (none, lambda k: ok(L.spl_dfa_step_device(h, ref(sib), ref(o), ref(sob), stream))),
                              "c_b": (none, lambda k: ok(L.spl_dfa_jump_device(h, ref(sib), ref(o), ref(sob), ref(jb), stream)))})
            assert int(flen.min().item()) > 0, "a sequence of (b) was not in a forced state"
            emit()
            emit(f"  -- {name}, B = {B}, K = 1: {B * nw * 4 / 1e6:.1f} MB of mask a call")
            m0, sp0 = line("(s0) spl_dfa_step_device, one drawn id a sequence", e["s0"])
            ma, spa = line("(a)  spl_dfa_jump_device, the same ids, a jump index of zeros", e["a"])
            emit(f"  -> (a) - (s0) = {(ma - m0) * 1e3:+.2f} us against the two spreads {sp0 * 1e3:.2f} and {spa * 1e3:.2f} us")
            mb0, _ = line("(b0) spl_dfa_step_device, no ids, every sequence in the start state", e["b0"])
            mb, _ = line(f"(b)  spl_dfa_jump_device, no ids, every sequence forced: {int(flen[0].item())} ids emitted each", e["b"])
            emit(f"  -> (b) - (b0) = {(mb - mb0) * 1e3:+.2f} us for {int(flen.sum().item())} emitted ids")
            summary.append(f"step {name} B={B}, the Python wrappers: step {m0 * 1e3:.2f} us, jump with a zero index {ma * 1e3:.2f} us ({(ma - m0) * 1e3:+.2f}), "
                           f"forced: step {mb0 * 1e3:.2f} us, jump {mb * 1e3:.2f} us ({(mb - mb0) * 1e3:+.2f})")
            emit("  the same through the C ABI, the structs built once:")
            c0, cs0 = line("(s0) spl_dfa_step_device, one drawn id a sequence", e["c_s0"])
            ca, csa = line("(a)  spl_dfa_jump_device, the same ids, a jump index of zeros", e["c_a"])
            emit(f"  -> (a) - (s0) = {(ca - c0) * 1e3:+.2f} us against the two spreads {cs0 * 1e3:.2f} and {csa * 1e3:.2f} us")
            cb0, _ = line("(b0) spl_dfa_step_device, no ids, every sequence in the start state", e["c_b0"])
            cb, _ = line("(b)  spl_dfa_jump_device, no ids, every sequence forced", e["c_b"])
            emit(f"  -> (b) - (b0) = {(cb - cb0) * 1e3:+.2f} us")
            summary.append(f"step {name} B={B}, the C ABI: step {c0 * 1e3:.2f} us, jump with a zero index {ca * 1e3:.2f} us ({(ca - c0) * 1e3:+.2f}), "
                           f"forced: step {cb0 * 1e3:.2f} us, jump {cb * 1e3:.2f} us ({(cb - cb0) * 1e3:+.2f})")
        # the draws
        with_jump, texts = draws(tok, special, by_id, True)
        without, _ = draws(tok, special, by_id, False)
        emit()
        emit(f"  (d) the draws, 256 sequences of the JSON pattern, uniform sampler: {with_jump} with jump, {without} without: "
             f"{(without - with_jump) / 256:.1f} forward passes saved an answer ({with_jump / 256:.1f} against {without / 256:.1f}); e.g. {texts[0]!r}")
        summary.append(f"draws {name}: {with_jump / 256:.2f} an answer with jump, {without / 256:.2f} without")
    emit()
    emit("summary")
    for s in summary:
        emit("  " + s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
