"""`Tokenizer`: the reference's Python surface over the HIP backend.

Mirrors the PyO3 class `Tokenizer` of the reference (src/python/bindings.rs:57-446) method for
method for the encode path: same names, argument meaning, return shapes and error behaviour.
Every encode call goes through the C ABI (include/splintr_hip.h) into the gfx950 kernels; there
is no CPU implementation in this package.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
_DATA = os.path.join(_HERE, "data")

# Verbatim pattern strings exported by the reference module (src/lib.rs:42-44,
# src/core/tokenizer.rs:39, :42, :45).  The HIP backend implements exactly these two.
CL100K_BASE_PATTERN = (
    r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"
)
O200K_BASE_PATTERN = (
    r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
    r"|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
    r"|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"
)
LLAMA3_PATTERN = O200K_BASE_PATTERN
MISTRAL_V3_PATTERN = (
    r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+"
    r"|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*"
    r"|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+"
)
# The GPU scanner implements exactly these patterns; any other pattern is SPL_PATTERN_CUSTOM: its split runs on the
# host cores (csrc/spl_regex.cpp) and feeds the same probe / merge kernels.
_PATTERN_ID = {CL100K_BASE_PATTERN: 0, O200K_BASE_PATTERN: 1, MISTRAL_V3_PATTERN: 2}

# name -> (vocab container, pattern, special-token table key)      src/python/bindings.rs:101-160
_PRETRAINED = {
    "cl100k_base": ("cl100k_base.splv", CL100K_BASE_PATTERN, "cl100k_base"),
    "o200k_base": ("o200k_base.splv", O200K_BASE_PATTERN, "o200k_base"),
    "llama3": ("llama3.splv", LLAMA3_PATTERN, "llama3"),
    "llama3.1": ("llama3.splv", LLAMA3_PATTERN, "llama3"),
    "llama3.2": ("llama3.splv", LLAMA3_PATTERN, "llama3"),
    "llama3.3": ("llama3.splv", LLAMA3_PATTERN, "llama3"),
    "deepseek_v3": ("deepseek_v3.splv", LLAMA3_PATTERN, "deepseek_v3"),
    "deepseek-v3": ("deepseek_v3.splv", LLAMA3_PATTERN, "deepseek_v3"),
    "mistral_v3": ("mistral_v3.splv", MISTRAL_V3_PATTERN, "mistral_v3"),
}


def _byte_level_alphabet() -> List[str]:
    """byte -> char of the GPT-2 ByteLevel alphabet (src/core/byte_level.rs:46-74)."""
    direct = set(range(33, 127)) | set(range(161, 173)) | set(range(174, 256))
    out, nxt = [], 256
    for b in range(256):
        if b in direct:
            out.append(chr(b))
        else:
            out.append(chr(nxt))
            nxt += 1
    return out


_BYTE_TO_CHAR = _byte_level_alphabet()


def _unicode_table_path(which: str) -> str:
    if which == "pcre2":
        return os.path.join(_DATA, "unicode_classes.bin")
    if which == "regex":
        return os.path.join(_DATA, "unicode_classes_regex.bin")
    return which


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _pack(texts: Sequence[str]):
    """list[str] -> (uint8 buffer, uint64 offsets), plain Python (DeviceBatch, tests).  TypeError for
    anything that is not a sequence of str (PyO3 refuses a bare str for Vec<String>;
    src/python/bindings.rs:337)."""
    if isinstance(texts, (str, bytes)):
        raise TypeError("Can't extract `str` to `Vec`")
    parts = []
    for t in texts:
        if not isinstance(t, str):
            raise TypeError(f"argument 'texts': '{type(t).__name__}' object cannot be converted to 'PyString'")
        parts.append(t.encode("utf-8"))          # lone surrogates -> UnicodeEncodeError, as in PyO3
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        np.cumsum([len(p) for p in parts], out=off[1:])
    buf = b"".join(parts)
    return buf, off


class Tokenizer:
    r"""The reference's `splintr.Tokenizer` surface on the MI355X backend: same constructor
    arguments (a tiktoken-format vocabulary file, a pattern, a special-token map), same methods.

    Differences from the reference, all refused loudly rather than approximated:
    * `pattern`: CL100K_BASE_PATTERN, O200K_BASE_PATTERN (= LLAMA3_PATTERN) and MISTRAL_V3_PATTERN are split on the
      GPU by closed-form scanners; any other pattern is compiled by the library's own regex matcher and run at every text position
      on the GPU (csrc/spl_rx_split.h; on the host cores for the rare DOCUMENT the device matcher gives up
      on -- a match longer than ~1 KB -- while the rest of its batch keeps the device split) (literals, classes, \s \d \w,
      every general category and every script as \p{..} / \P{..}, groups, (?i:), (?>), alternation, greedy / lazy / possessive
      quantifiers, look-ahead, ^ $ \A \Z \z \b \B: upstream tiktoken's cl100k_base / o200k_base strings, Qwen2's, GPT-2's and
      \p{Han}-style patterns are accepted as they are) and merged on the GPU; a pattern with anything else in it (binary
      properties, script extensions, look-behind, back-references, \p{Lu} under (?i)) or one that can match the empty string
      raises the reference's "Regex error" ValueError naming the construct;
    * the vocabulary must contain all 256 single bytes and ids below 2**21 - 1;
    * every key of up to 8 bytes gets a table slot of its own by hash-and-displace (csrc/spl_tables.cpp): a vocabulary in
      which so many such keys share one two-byte prefix (keys of 1..4 bytes: 16-bit salt) or one four-byte-prefix filter slot
      (keys of 5..8 bytes: 10-bit salt) that no salt separates them even after the table was doubled three times is refused
      ("could not give every key ... a slot of its own").  None of the pretrained or tested vocabularies comes near it
      (largest group: 256 keys); the reference's FxHashMap has no such limit;
    * special-token literals are at most 255 bytes (any set: literals that contain or chain into one
      another are matched as the reference's Aho-Corasick matcher does).
    Extensions: `device=` / `devices=` select the GPU(s), `byte_level=True` is the reference's
    `from_bytes_byte_level`; the vocabulary may also be this repo's packed SPLV container.
    `unicode_tables=`: which Unicode character data \p{L} \p{N} \s ... mean -- "pcre2" (default: probed from PCRE2 10.39,
    Unicode 14.0, the engine the reference's own tests declare equivalent to its default one), "regex" (probed from the
    Python `regex` module, a newer Unicode: 14 186 code points are classed differently, U+180E among them), or the path
    of a table made by tools/gen_unicode_tables.py.  The reference's default engine (regexr, Cargo.toml:41) ships tables
    of a version that cannot be determined here; nothing in the reference pins the difference.
    """

    def __init__(self, vocab_path: str, pattern: str, special_tokens: Optional[Dict[str, int]] = None, *,
                 device: int = 0, byte_level: bool = False, unicode_tables: str = "pcre2"):
        # src/python/bindings.rs:70-83: every failure of from_file surfaces as IOError
        try:
            blob = _read(vocab_path)
            self._init_from_blob(blob, pattern, special_tokens or {}, device, byte_level, unicode_tables)
        except (OSError, ValueError) as e:
            raise IOError(str(e)) from None

    # ------------------------------------------------------------------ construction
    def _init_from_blob(self, blob: bytes, pattern: str, special_tokens: Dict[str, int], device: int,
                        byte_level: bool = False, unicode_tables: str = "pcre2"):
        if not isinstance(pattern, str):
            raise TypeError("argument 'pattern': object cannot be converted to 'PyString'")
        L = _ffi.lib()
        ucls = _read(_unicode_table_path(unicode_tables))
        flags = _ffi.SPL_OPT_BYTE_LEVEL if byte_level else 0
        if pattern in _PATTERN_ID:
            opts = _ffi.SplOpts(_PATTERN_ID[pattern], device, flags)
        else:                                   # src/core/tokenizer.rs:426: any pattern is compiled
            self._pattern_bytes = pattern.encode("utf-8")
            opts = _ffi.SplOpts(_ffi.SPL_PATTERN_CUSTOM, device, flags, self._pattern_bytes)
        self._h = L.spl_create(blob, len(blob), ucls, len(ucls), ctypes.byref(opts))
        if not self._h:
            raise ValueError(_ffi.last_error())
        self._device = device
        self._pattern = pattern
        self._special = dict(special_tokens)
        for lit, tid in self._special.items():
            b = lit.encode("utf-8")
            if L.spl_add_special(self._h, b, len(b), int(tid)) != 0:
                raise ValueError(_ffi.last_error())

    @classmethod
    def _from_blob(cls, blob: bytes, pattern: str, special_tokens: Dict[str, int], device: int = 0,
                   byte_level: bool = False, unicode_tables: str = "pcre2") -> "Tokenizer":
        self = cls.__new__(cls)
        self._init_from_blob(blob, pattern, special_tokens, device, byte_level, unicode_tables)
        return self

    @staticmethod
    def from_pretrained(name: str, device: int = 0, unicode_tables: str = "pcre2") -> "Tokenizer":
        """src/python/bindings.rs:101-166 (in-scope names: cl100k_base, o200k_base, llama3*,
        deepseek_v3 / deepseek-v3)."""
        if not isinstance(name, str):
            raise TypeError("argument 'name': object cannot be converted to 'PyString'")
        ent = _PRETRAINED.get(name)
        if ent is None:
            raise ValueError(
                f"Unknown pretrained model: {name}. See from_pretrained docstring for supported models.")
        fn, pattern, skey = ent
        with open(os.path.join(_DATA, "special_tokens.json"), encoding="utf-8") as f:
            special = json.load(f)[skey]
        return Tokenizer._from_blob(_read(os.path.join(_DATA, fn)), pattern, special, device, False, unicode_tables)

    @staticmethod
    def from_bytes(vocab_data: bytes, pattern: str, special_tokens: Optional[Dict[str, int]] = None,
                   device: int = 0, unicode_tables: str = "pcre2") -> "Tokenizer":
        """src/python/bindings.rs:174-187: `vocab_data` is tiktoken text (`base64 rank` lines), as in
        the reference; this repo's SPLV container is accepted as well."""
        return Tokenizer._from_blob(bytes(vocab_data), pattern, special_tokens or {}, device, False, unicode_tables)

    @staticmethod
    def from_bytes_byte_level(vocab_data: bytes, pattern: str, special_tokens: Optional[Dict[str, int]] = None,
                              device: int = 0, unicode_tables: str = "pcre2") -> "Tokenizer":
        """src/core/tokenizer.rs:562-569 (not exposed by the reference's Python class; used by its
        from_pretrained for deepseek_v3 and mistral_v3)."""
        return Tokenizer._from_blob(bytes(vocab_data), pattern, special_tokens or {}, device, True, unicode_tables)

    def set_devices(self, devices: Sequence[int]) -> "Tokenizer":
        """Extension: spread `encode_batch` over several GPUs from this one process
        (spl_set_devices: documents sharded by bytes, one pinned CSR result)."""
        arr = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
        if _ffi.lib().spl_set_devices(self._h, arr, len(devices)) != 0:
            raise ValueError(_ffi.last_error())
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _ffi.lib().spl_destroy(h)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------ encode path
    def _encode_packed(self, buf, off, nd: int, flags: int):
        """C-ABI call: packed UTF-8 + offsets in (objects or addresses), CSR (ids uint32, offsets
        uint64) out as numpy arrays."""
        L = _ffi.lib()
        res = ctypes.c_void_p()
        rc = L.spl_encode_batch(self._h, buf, off, nd, flags, ctypes.byref(res))
        if rc != 0:
            raise RuntimeError(f"spl_encode_batch failed ({rc}): {_ffi.last_error()}")
        try:
            nt = L.spl_result_n_tokens(res)
            ids = (np.ctypeslib.as_array(L.spl_result_tokens(res), shape=(nt,)).copy() if nt
                   else np.zeros(0, dtype=np.uint32))
            oo = np.ctypeslib.as_array(L.spl_result_offsets(res), shape=(nd + 1,)).copy()
        finally:
            L.spl_result_free(res)
        return ids, oo

    def encode_packed(self, utf8: bytes, offsets: np.ndarray, with_special: bool = False):
        """Extension: the C-ABI call on an already packed corpus (bytes + uint64 offsets[N+1])."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        return self._encode_packed(utf8, offsets.ctypes.data, len(offsets) - 1,
                                   _ffi.SPL_WITH_SPECIAL if with_special else 0)

    def encode_batch_csr(self, texts: Sequence[str], with_special: bool = False):
        """Extension: the batch result as CSR numpy arrays (ids uint32[T], offsets uint64[N+1])
        without materialising Python lists."""
        # ONE C call with the GIL held (staging, spl_encode_batch, copy out): safe from several threads
        ids, off = _ffi.shim().encode_batch_csr(self._h, texts, _ffi.SPL_WITH_SPECIAL if with_special else 0)
        return np.frombuffer(ids, dtype=np.uint32), np.frombuffer(off, dtype=np.uint64)

    def _encode_one(self, text: str, flags: int) -> List[int]:
        return _ffi.shim().encode(self._h, text, flags)

    def encode(self, text: str) -> List[int]:
        """src/python/bindings.rs:254-256.  Texts of up to 4 KB take the library's latency path (csrc/spl_pipeline.h encode_small: no copy
        engine, no stream synchronisation -- the tile kernel reads the text from pinned host memory, the host spins on a completion word)."""
        return _ffi.shim().encode(self._h, text, 0)

    def encode_rayon(self, text: str) -> List[int]:
        """src/python/bindings.rs:273-275: same ids as encode (the GPU path is always
        chunk-parallel inside a text)."""
        return self._encode_one(text, _ffi.SPL_INTRA_DOC)

    def encode_with_special(self, text: str) -> List[int]:
        """src/python/bindings.rs:286-288."""
        return self._encode_one(text, _ffi.SPL_WITH_SPECIAL)

    def _batch(self, texts: Sequence[str], flags: int) -> List[List[int]]:
        # ONE C call: UTF-8 straight into pinned staging, spl_encode_batch, lists from the pinned CSR
        return _ffi.shim().encode_batch(self._h, texts, flags)

    def encode_batch(self, texts: Sequence[str]) -> List[List[int]]:
        """src/python/bindings.rs:337-339."""
        return self._batch(texts, 0)

    def encode_batch_with_special(self, texts: Sequence[str]) -> List[List[int]]:
        """src/python/bindings.rs:348-350."""
        return self._batch(texts, _ffi.SPL_WITH_SPECIAL)

    # ------------------------------------------------------------------ tokens a model on the same GPU reads (device tensors)
    def _encode_on_device(self, texts: Sequence[str], with_special: bool):
        import torch                                 # (lazily: this module imports without torch)
        from . import device as dv
        batch = dv.DeviceBatch(texts, torch.device("cuda", self._device))
        dv.encode_device(self, batch, with_special)
        return dv, batch

    def encode_batch_padded(self, texts: Sequence[str], max_length: int, *, pad_id: int, with_special: bool = False,
                            bos_id: Optional[int] = None, eos_id: Optional[int] = None, padding_side: str = "right",
                            truncation_side: str = "right", dtype=None):
        """Extension: encode_batch as a dense batch ON THE GPU -- (input_ids [n_docs, max_length], attention_mask uint8, lengths int32),
        torch tensors on this tokenizer's device; dtype torch.int32 (default) or torch.int64.  The texts go to the device, the encode
        and ONE more launch (splintr_amd.device.pad_device) run on torch's current stream, nothing synchronises in between."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_collate_args(max_length, pad_id, bos_id, eos_id, dtype, padding_side, truncation_side)   # (before anything goes to the device)
        dv, batch = self._encode_on_device(texts, with_special)
        return dv.pad_device(self, batch, max_length, pad_id=pad_id, bos_id=bos_id, eos_id=eos_id, padding_side=padding_side,
                             truncation_side=truncation_side, dtype=dtype)

    def encode_batch_packed(self, texts: Sequence[str], seq_len: int, *, pad_id: int, with_special: bool = False,
                            bos_id: Optional[int] = None, eos_id: Optional[int] = None, dtype=None):
        """Extension: encode_batch as packed sequences ON THE GPU -- the documents, each as [bos_id] ids [eos_id], joined into one
        stream and cut into rows of seq_len: (rows [n_rows, seq_len], doc_ids int32, positions int32); the tail of the last row holds
        pad_id (doc_ids -1).  Positions restart at every document and every row.  ONE synchronisation, to learn n_rows."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_collate_args(seq_len, pad_id, bos_id, eos_id, dtype)        # (before anything goes to the device)
        dv, batch = self._encode_on_device(texts, with_special)
        rows, doc, pos, n = dv.pack_device(self, batch, seq_len, pad_id=pad_id, bos_id=bos_id, eos_id=eos_id,
                                           dtype=dtype)
        n_rows = int(n[0].item())
        return rows[:n_rows], doc[:n_rows], pos[:n_rows]

    def encode_batch_windows(self, texts: Sequence[str], max_length: int, *, overlap: int = 0, pad_id: int, with_special: bool = False,
                             bos_id: Optional[int] = None, eos_id: Optional[int] = None, padding_side: str = "right", dtype=None):
        """Extension: encode_batch as SLIDING WINDOWS ON THE GPU -- every document alone and complete, as rows of max_length whose
        bodies overlap by `overlap` ids (Hugging Face's name for `overlap` is `stride`, with return_overflowing_tokens): (input_ids
        [n_rows, max_length], attention_mask uint8, lengths int32 [n_rows], doc_ids int32 [n_rows], starts int64 [n_rows], row_offsets
        int64 [n_docs + 1]).  Row r is a window of document doc_ids[r] that begins at id starts[r] of it; the rows of document d are
        row_offsets[d] .. row_offsets[d + 1] - 1.  BOS and EOS are on every row.  ONE synchronisation, to learn n_rows."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_window_args(max_length, overlap, pad_id, bos_id, eos_id, dtype, padding_side)   # (before anything goes to the device)
        dv, batch = self._encode_on_device(texts, with_special)
        rows, mask, lens, doc, start, row_off, n = dv.window_device(self, batch, max_length, overlap=overlap, pad_id=pad_id, bos_id=bos_id,
                                                                    eos_id=eos_id, padding_side=padding_side, dtype=dtype)
        n_rows = int(n[0].item())
        return rows[:n_rows], mask[:n_rows], lens[:n_rows], doc[:n_rows], start[:n_rows], row_off

    def encode_batch_pairs(self, texts_a: Sequence[str], texts_b: Sequence[str], max_length: int, *, pad_id: int, cross: bool = False,
                           a_index=None, b_index=None, with_special: bool = False, prefix=(), middle=(), suffix=(),
                           truncation: str = "longest_first", truncation_side_a: str = "right", truncation_side_b: str = "right",
                           padding_side: str = "right", dtype=None, check: bool = False):
        """Extension: PAIRS of texts as one row each ON THE GPU (Hugging Face's text_pair) -- row p = prefix + A' + middle + B' + suffix
        padded to max_length, the two texts encoded SEPARATELY (joining the strings first changes the tokens at the seam) and cut to the
        row by `truncation` ("longest_first", "only_first", "only_second"; the fixed segments are never cut away).  texts_a + texts_b
        are ONE device batch and one encode; one more launch (splintr_amd.device.pair_device) builds the rows from its two slices.  By
        default pair i = (texts_a[i], texts_b[i]) and the two lists must be equally long; cross=True builds the whole len(a) x len(b)
        grid, row i * len(b) + j = (a_i, b_j) -- a query is encoded once however many candidates it meets; a_index / b_index (int32
        device tensors or sequences) name each pair's texts themselves.  Returns (input_ids [n_pairs, max_length], attention_mask uint8,
        token_type_ids uint8, special_tokens_mask uint8, lengths int32 [n_pairs], kept int32 [n_pairs, 2], status int32 [1]), torch
        tensors on this tokenizer's device; nothing synchronises.  An index that names no text gives an empty side and status[0] = 1;
        check=True reads status (ONE synchronisation) and raises IndexError instead."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_pair_args(max_length, pad_id, prefix, middle, suffix, truncation, truncation_side_a, truncation_side_b, padding_side,
                           dtype)                    # (before anything goes to the device)
        for name, texts in (("texts_a", texts_a), ("texts_b", texts_b)):
            if isinstance(texts, (str, bytes)) or not hasattr(texts, "__len__"):
                raise ValueError(f"{name} must be a sequence of str, not {type(texts).__name__}")
        n_a, n_b = len(texts_a), len(texts_b)
        if cross and (a_index is not None or b_index is not None):
            raise ValueError("cross=True builds both index arrays itself: give it, or a_index / b_index, not both")
        if not cross and a_index is None and b_index is None and n_a != n_b:
            raise ValueError(f"pair i is (texts_a[i], texts_b[i]): the lists must be equally long, not {n_a} and {n_b} "
                             "(cross=True pairs every a with every b; a_index / b_index name the pairs)")
        if cross and n_a * n_b >= (1 << 31):
            raise ValueError("cross=True: the grid must hold fewer than 2**31 pairs")
        dv, batch = self._encode_on_device(list(texts_a) + list(texts_b), with_special)
        dev = batch.ids.device
        if cross:                                    # (made on the device: nothing is copied, nothing synchronises)
            a_index = torch.arange(n_a, dtype=torch.int32, device=dev).repeat_interleave(n_b)
            b_index = torch.arange(n_b, dtype=torch.int32, device=dev).repeat(n_a)
        out = dv.pair_csr_device(self, batch.ids, batch.out_off, n_a, batch.ids, batch.out_off[n_a:], n_b, max_length, pad_id=pad_id,
                                 prefix=prefix, middle=middle, suffix=suffix, a_index=a_index, b_index=b_index, truncation=truncation,
                                 truncation_side_a=truncation_side_a, truncation_side_b=truncation_side_b, padding_side=padding_side,
                                 dtype=dtype)
        if check and int(out[-1].item()):
            raise IndexError(f"encode_batch_pairs: an entry of a_index / b_index names no text (valid: 0 .. {n_a - 1} for a, 0 .. {n_b - 1} for b)")
        return out

    def encode_batch_chat(self, conversations, max_length: int, *, template, pad_id: int, add_generation_prompt: bool = False,
                          truncation: str = "right", pin_system: bool = False, padding_side: str = "right", ignore_index: int = -100,
                          train_turns=None, with_special: bool = False, dtype=None, check: bool = False):
        """Extension: multi-turn CONVERSATIONS as one row each ON THE GPU, with labels (Hugging Face's apply_chat_template with
        tokenize=True and return_assistant_tokens_mask=True).  conversations: a sequence of sequences of {"role", "content"} dicts or
        (role, content) tuples; template: a splintr_amd.chat.ChatTemplate (ChatTemplate.chatml(tok), ChatTemplate.llama3(tok)).  Row c
        = bos + per turn (the role's header + the message's ids + the role's footer) + the generation prompt (add_generation_prompt),
        padded to max_length.  Every message is encoded by itself and equal message strings ONCE (a shared system prompt is one
        document of the device batch); the control tokens come from the template, so with with_special=False, the default, message
        text that spells <|eot_id|> stays ordinary text and cannot forge a turn.  truncation "right" cuts the body at the row's end,
        "drop_oldest" removes whole turns from the front (pin_system keeps turn 0).  train_turns: per conversation one truth value per
        turn, False takes that turn's labels away.  Returns splintr_amd.device.ChatRows (input_ids, labels, attention_mask, role_ids,
        loss_mask, special_tokens_mask, lengths, kept, turn_cols, status), torch tensors on this tokenizer's device; nothing
        synchronises.  check=True reads status (ONE synchronisation) and raises IndexError if it is set."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_chat_args(max_length, pad_id, template, add_generation_prompt, truncation, pin_system, padding_side, ignore_index,
                           dtype)                    # (before anything goes to the device)
        texts, turn_doc, turn_role, turn_train, conv_off = dv.chat_turns(conversations, template, train_turns)
        dv, batch = self._encode_on_device(texts, with_special)
        dev = batch.ids.device
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        out = dv.chat_device(self, batch, up(turn_doc), up(turn_role), up(conv_off), max_length, template=template, pad_id=pad_id,
                             add_generation_prompt=add_generation_prompt, truncation=truncation, pin_system=pin_system,
                             padding_side=padding_side, ignore_index=ignore_index, turn_train=up(turn_train), dtype=dtype)
        if check and int(out.status.item()):
            raise IndexError("encode_batch_chat: a role, a document index or a turn range was out of range")
        return out

    def encode_batch_chat_packed(self, conversations, seq_len: int, *, template, pad_id: int, strategy: str = "best_fit_decreasing",
                                 add_generation_prompt: bool = False, truncation: str = "right", pin_system: bool = False,
                                 ignore_index: int = -100, train_turns=None, with_special: bool = False, dtype=None, mask_first: bool = True,
                                 max_rows: Optional[int] = None, trim: bool = True, check: bool = False):
        """Extension: encode_batch_chat PACKED ON THE GPU for fine-tuning -- several whole conversations per row of seq_len, none cut in
        two (torchtune's PackedDataset, TRL's packing): encode_batch_chat with max_length = seq_len, then
        splintr_amd.device.seqpack_rows_device over its rows; labels, loss_mask, role_ids and special_tokens_mask travel along.  strategy
        "best_fit_decreasing" (fewest rows; seq_len <= 32768) or "next_fit" (keeps the order).  mask_first: the label at every
        conversation's first column is ignore_index.  Returns splintr_amd.device.PackedRows (input_ids, labels, attention_mask,
        position_ids, seq_ids, loss_mask, role_ids, special_tokens_mask, extra (None), seq_place, row_fill, cu_seqlens, n, status).  trim
        (default) cuts the tensors to the rows used and cu_seqlens to its entries: ONE synchronisation; trim=False returns [max_rows,
        seq_len] tensors (max_rows defaults to the number of conversations) and synchronises nothing.  check=True raises IndexError if
        encode_batch_chat's status is set."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_seqpack_args(seq_len, pad_id=pad_id, strategy=strategy, ignore_index=ignore_index, mask_first=mask_first, dtype=dtype,
                              max_rows=max_rows)       # (before anything goes to the device)
        rows = self.encode_batch_chat(conversations, seq_len, template=template, pad_id=pad_id, add_generation_prompt=add_generation_prompt,
                                      truncation=truncation, pin_system=pin_system, ignore_index=ignore_index, train_turns=train_turns,
                                      with_special=with_special, dtype=dtype, check=check)
        out = dv.seqpack_rows_device(self, rows.input_ids, rows.lengths, seq_len, pad_id=pad_id, strategy=strategy, labels=rows.labels,
                                     loss_mask=rows.loss_mask, role_ids=rows.role_ids, special_tokens_mask=rows.special_tokens_mask,
                                     ignore_index=ignore_index, mask_first=mask_first, max_rows=max_rows)
        return dv.seqpack_trim(out) if trim else out

    def encode_batch_packed_whole(self, texts: Sequence[str], seq_len: int, *, pad_id: int, bos_id: Optional[int] = None,
                                  eos_id: Optional[int] = None, strategy: str = "best_fit_decreasing", truncation_side: str = "right",
                                  with_special: bool = False, dtype=None, max_rows: Optional[int] = None, trim: bool = True):
        """Extension: encode_batch as packed rows ON THE GPU with every document WHOLE -- [bos_id] ids [eos_id] of several documents per
        row of seq_len, none cut in two (encode_batch_packed cuts one stream every seq_len instead).  A document longer than seq_len
        is truncated (BOS and EOS are never cut away).  Returns splintr_amd.device.PackedRows without labels and byte arrays; seq_ids
        are document numbers, cu_seqlens what a varlen attention call takes.  trim as for encode_batch_chat_packed."""
        import torch
        from . import device as dv
        dtype = torch.int32 if dtype is None else dtype
        dv.check_collate_args(seq_len, pad_id, bos_id, eos_id, dtype, "right", truncation_side)
        dv.check_seqpack_args(seq_len, pad_id=pad_id, strategy=strategy, truncation_side=truncation_side, dtype=dtype, max_rows=max_rows)
        dv, batch = self._encode_on_device(texts, with_special)
        if bos_id is None and eos_id is None:           # the CSR as it is
            out = dv.seqpack_csr_device(self, batch.ids, batch.out_off, batch.n_docs, seq_len, pad_id=pad_id, strategy=strategy,
                                        truncation_side=truncation_side, dtype=dtype, max_rows=max_rows)
        else:                                           # BOS and EOS join a document in pad_device's rows
            rows, _, lens = dv.pad_device(self, batch, seq_len, pad_id=pad_id, bos_id=bos_id, eos_id=eos_id, truncation_side=truncation_side,
                                          dtype=dtype)
            out = dv.seqpack_rows_device(self, rows, lens, seq_len, pad_id=pad_id, strategy=strategy, max_rows=max_rows)
        return dv.seqpack_trim(out) if trim else out

    def encode_batch_with_offsets(self, texts: Sequence[str], *, unit: str = "char", with_special: bool = False):
        """Extension: encode_batch plus WHERE every token lies in its text -- (ids list[list[int]], spans list[list[(start, end)]]), a
        span in characters (unit="char": Python str indices, Hugging Face's offset_mapping; a token that begins inside a character
        starts at that character -- tiktoken's decode_with_offsets -- and ends behind the last character it touches) or in bytes of the
        UTF-8 text (unit="byte": text.encode()[start:end] is the token).  The encode and the spans (splintr_amd.device.spans_device)
        run on the device on torch's current stream; the offsets come back first (the one synchronisation), then the ids and the spans
        of exactly the tokens there are in one copy.  ValueError naming the first document whose ids do not decode to its text (a custom
        pattern that leaves gaps, a vocabulary that lacks a byte): its spans would not index the text."""
        if unit not in ("char", "byte"):
            raise ValueError(f"unit must be 'char' or 'byte', not {unit!r}")
        import torch
        dv, batch = self._encode_on_device(texts, with_special)
        byte_span, char_span, byte_off, _ = dv.spans_device(self, batch.ids, batch.out_off, chars=unit == "char")
        off = torch.stack([batch.out_off, byte_off]).cpu().numpy()
        tok_off, got = off[0], np.diff(off[1])
        want = np.diff(batch.host_offsets.astype(np.int64))
        if not np.array_equal(got, want):
            d = int(np.argmax(got != want))
            raise ValueError(f"encode_batch_with_offsets: document {d} is {int(want[d])} bytes of UTF-8 but its ids decode to {int(got[d])}: "
                             "the encode dropped or changed bytes, spans would not index the text")
        n = int(tok_off[-1])
        span = char_span if unit == "char" else byte_span
        flat = torch.cat([batch.ids[:n].reshape(n, 1), span[:n]], dim=1).cpu().numpy()
        ids, spans = flat[:, 0].view(np.uint32).tolist(), list(zip(flat[:, 1].tolist(), flat[:, 2].tolist()))
        cuts = tok_off.tolist()
        return [ids[a:b] for a, b in zip(cuts, cuts[1:])], [spans[a:b] for a, b in zip(cuts, cuts[1:])]

    def decode_with_offsets(self, tokens: Sequence[int]):
        """tiktoken's decode_with_offsets: (text, the character index at which each token starts); a token that begins inside a
        character starts at that character.  Strict as decode (ValueError on invalid UTF-8); an id of neither map contributes nothing
        and starts where the next token does.  The starts come from the device (splintr_amd.device.spans_rows_device, one row)."""
        text = self.decode(tokens)
        if not len(tokens):
            return text, []
        import torch
        from . import device as dv
        row = torch.tensor([list(tokens)], dtype=torch.int64, device=torch.device("cuda", self._device))
        _, char_span, _, _ = dv.spans_rows_device(self, row)
        return text, char_span[:, 0].cpu().tolist()

    # ------------------------------------------------------------------ decode (test helper / "next" row)
    def decode_bytes(self, tokens: Sequence[int]) -> bytes:
        """src/python/bindings.rs:313-315."""
        return self._decode_batch_bytes([tokens])[0]

    def _decode_batch_bytes(self, token_lists: Sequence[Sequence[int]]) -> List[bytes]:
        L = _ffi.lib()
        off = np.zeros(len(token_lists) + 1, dtype=np.uint64)
        if len(token_lists):
            np.cumsum([len(t) for t in token_lists], out=off[1:])
        ids = np.fromiter((x for t in token_lists for x in t), dtype=np.uint32, count=int(off[-1]))
        ob = ctypes.POINTER(ctypes.c_uint8)()
        oo = ctypes.POINTER(ctypes.c_uint64)()
        rc = L.spl_decode_batch(self._h, ids.ctypes.data, off.ctypes.data, len(token_lists), ctypes.byref(ob),
                                ctypes.byref(oo))
        if rc != 0:
            raise RuntimeError(f"spl_decode_batch failed ({rc}): {_ffi.last_error()}")
        try:
            o = [oo[i] for i in range(len(token_lists) + 1)]
            raw = ctypes.string_at(ob, o[-1]) if o[-1] else b""
        finally:
            L.spl_free(ob)
            L.spl_free(oo)
        return [raw[o[i]:o[i + 1]] for i in range(len(token_lists))]

    def decode(self, tokens: Sequence[int]) -> str:
        """src/python/bindings.rs:300-304 (ValueError on invalid UTF-8)."""
        try:
            return self.decode_bytes(tokens).decode("utf-8")
        except UnicodeDecodeError:
            raise ValueError("Decoding error: invalid UTF-8") from None

    def decode_lossy(self, tokens: Sequence[int]) -> str:
        return self.decode_bytes(tokens).decode("utf-8", "replace")

    def decode_batch(self, token_lists: Sequence[Sequence[int]]) -> List[str]:
        try:
            return [b.decode("utf-8") for b in self._decode_batch_bytes(token_lists)]
        except UnicodeDecodeError:
            raise ValueError("Decoding error: invalid UTF-8") from None

    def decode_batch_lossy(self, token_lists: Sequence[Sequence[int]]) -> List[str]:
        return [b.decode("utf-8", "replace") for b in self._decode_batch_bytes(token_lists)]

    def decode_tensor(self, input_ids, lengths=None, *, padding_side: str = "right", skip_special_tokens: bool = False,
                      errors: str = "strict") -> List[str]:
        """Extension: rows [batch, steps] of ids ON THE GPU (int32 / int64; lengths int32 [batch] or None, as encode_batch_padded
        returns them) to one str per row.  The decode runs on the device (splintr_amd.device.decode_rows_device) into a buffer of 6
        bytes per id; the byte count it needed is read back, and only if the guess was short the decode runs once more with the exact
        size; then ONE copy of the bytes and one of the offsets to the host.  errors: "strict" (ValueError on invalid UTF-8, as decode)
        or "replace"."""
        from . import device as dv
        if errors not in ("strict", "replace"):
            raise ValueError(f"errors must be 'strict' or 'replace', not {errors!r}")
        dv.check_decode_args(input_ids, None, lengths, rows=True, padding_side=padding_side)      # (before anything goes to the device)
        kw = dict(padding_side=padding_side, skip_special_tokens=skip_special_tokens)
        out, off = dv.decode_rows_device(self, input_ids, lengths, max_bytes=6 * input_ids.numel(), **kw)
        need = int(off[-1].item())
        if need > out.numel():
            out, off = dv.decode_rows_device(self, input_ids, lengths, max_bytes=need, **kw)
        raw = out[:need].cpu().numpy().tobytes()
        o = off.cpu().tolist()
        try:
            return [raw[o[i]:o[i + 1]].decode("utf-8", errors) for i in range(len(o) - 1)]
        except UnicodeDecodeError:
            raise ValueError("Decoding error: invalid UTF-8") from None

    # ------------------------------------------------------------------ streaming decoders (host side)
    def _token_bytes(self, token_id: int, byte_level_decoded: bool) -> Optional[bytes]:
        """What the reference's decoder / special_tokens_decoder maps give for one id.
        byte_level_decoded False: the vocabulary KEY (ByteLevel text for ByteLevel vocabularies)."""
        if not 0 <= token_id < (1 << 32):
            return None
        L = _ffi.lib()
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        kind = L.spl_token_bytes(self._h, token_id, ctypes.byref(p), ctypes.byref(n))
        if kind == 0:
            return None
        b = ctypes.string_at(p, n.value) if n.value else b""
        if kind == 1 and not byte_level_decoded and L.spl_is_byte_level(self._h):
            b = "".join(_BYTE_TO_CHAR[x] for x in b).encode("utf-8")      # back to the key (byte_level.rs:105-107)
        return b

    def streaming_decoder(self):
        """src/python/bindings.rs:386-405."""
        from .streaming import StreamingDecoder
        return StreamingDecoder(lambda t: self._token_bytes(t, False))

    def byte_level_streaming_decoder(self):
        """src/python/bindings.rs:407-427."""
        from .streaming import ByteLevelStreamingDecoder
        return ByteLevelStreamingDecoder(lambda t: self._token_bytes(t, True))

    def device_streaming_decoder(self, batch_size: int, *, errors: str = "hold", skip_special_tokens: bool = False, stop=None,
                                 include_stop_str_in_output: bool = False):
        """Extension: batch_size streaming decoders whose state lives ON THE GPU (splintr_amd.device.DeviceStreamingDecoder): a sampler's
        step -- ids [B] or [B, K] as a device tensor -- goes in, the text that may leave comes back, one launch per step for small
        batches.  errors "hold": what byte_level_streaming_decoder (ByteLevel vocabularies) / streaming_decoder emit, step for step;
        "replace": U+FFFD for invalid bytes, no sequence ever stalls.  stop: up to 64 stop strings (str or bytes, 1 .. 64 bytes each): the
        text is cut at the first of them, what may still become one is held back, and `finished` / `stop_hit` stay on the device."""
        from . import device as dv
        return dv.DeviceStreamingDecoder(self, batch_size, errors=errors, skip_special_tokens=skip_special_tokens, stop=stop,
                                         include_stop_str_in_output=include_stop_str_in_output)

    def token_healer(self, batch_size: int, n_words: Optional[int] = None, max_back: int = 1, auto: bool = True):
        """Extension: token healing on the GPU (splintr_amd.device.TokenHealer): begin(rows, lengths) takes up to max_back tokens off
        every prompt's end, step(ids) follows the sampler, and `mask` -- int32 [B, n_words], the apply_token_bitmask layout -- holds the
        ids whose bytes agree with what was taken, until it is spelled again.  auto: a token is taken only if some token extends it."""
        from . import device as dv
        return dv.TokenHealer(self, batch_size, n_words=n_words, max_back=max_back, auto=auto)

    def choice_guide(self, batch_size: int, choices, *, end_ids=None, then_free: bool = False, n_words: Optional[int] = None):
        """Extension: guided choice on the GPU (splintr_amd.device.ChoiceGuide): the answer of every sequence is exactly one of up to 64
        `choices` (str or bytes, 1 .. 64 bytes each).  begin(selections) writes the candidate sets and the first masks, step(ids) follows
        the sampler, and `mask` -- int32 [B, n_words], the apply_token_bitmask layout -- holds the ids some remaining choice goes on with.
        end_ids: the ids (usually specials, up to 8) that may follow a choice that is spelled out and end the sequence; then_free: a
        sequence is done as soon as a choice is spelled out.  `done`, `hit`, `broken` and `spelled` read the state on the device."""
        from . import device as dv
        return dv.ChoiceGuide(self, batch_size, choices, end_ids=end_ids, then_free=then_free, n_words=n_words)

    def regex_guide(self, batch_size: int, pattern_or_patterns, *, end_ids, n_words: Optional[int] = None, jump: bool = False, jump_ids: int = 16):
        """Extension: the regex guide on the GPU (splintr_amd.device.RegexGuide): the answer of every sequence matches a regular
        expression -- Python `re` semantics in bytes mode, fullmatch; splintr_amd.dfa names what is supported.  A list of patterns is
        stacked into one table and begin(select) picks one per sequence.  begin() writes the start states and the first masks, step(ids)
        follows the sampler, and `mask` -- int32 [B, n_words], the apply_token_bitmask layout -- holds the ids the automaton can walk
        on with.  end_ids: the ids (usually specials, 1 .. 8) that may follow an accepting state and end the sequence.  `done`, `broken`
        and `live` read the state on the device.  jump=True adds jump-forward: jump(ids) is step(ids) that also returns, as ids
        (int32 [B, jump_ids] and their counts), the run the automaton forces behind them -- tokens that need no forward pass.
        Behind a speculative sampler: draft(ids, lengths, parent) gives, in one launch and without moving the guide, the mask in front of
        and behind every id of a draft chain or tree and whether each id is acceptable; accept(ids, lengths) commits."""
        from . import device as dv
        return dv.RegexGuide(self, batch_size, pattern_or_patterns, end_ids=end_ids, n_words=n_words, jump=jump, jump_ids=jump_ids)

    def nest_guide(self, batch_size: int, table, *, end_ids, max_depth: int = 64, n_words: Optional[int] = None):
        """Extension: the nest guide on the GPU (splintr_amd.device.NestGuide): the answer of every sequence is a word of a language made
        of regular pieces inside nested brackets, given as a splintr_amd.nest.NestTable -- a byte automaton whose transitions may push
        and pop a stack of at most max_depth (1 .. 64) 4-bit symbols per sequence.  begin() writes the start state and the first masks,
        step(ids) follows the sampler, `mask` holds the ids the next step may draw.  end_ids: the ids (usually specials, 1 .. 8) that
        may follow an accepting state with an empty stack and end the sequence.  `done`, `broken`, `live` and `depth` read the device.
        draft(ids, lengths, parent), accept and accept_node serve a speculative sampler as the regex guide's do."""
        from . import device as dv
        return dv.NestGuide(self, batch_size, table, end_ids=end_ids, max_depth=max_depth, n_words=n_words)

    def json_guide(self, batch_size: int, *, end_ids, top: str = "object", ws: str = "json", max_depth: int = 32, n_words: Optional[int] = None):
        """Extension: JSON MODE on the GPU -- the answer of every sequence is SOME valid JSON document (response_format json_object,
        guided_json without a schema): nest_guide over splintr_amd.nest.json_table(top, ws).  top: "object" (the usual contract),
        "array" or "value"; ws: "json" (any whitespace JSON allows), "compact" (at most one space after , and :) or "none";
        max_depth: the deepest nesting the masks allow."""
        from . import nest
        return self.nest_guide(batch_size, nest.json_table(top, ws), end_ids=end_ids, max_depth=max_depth, n_words=n_words)

    def apply_token_bitmask(self, logits, mask, *, live=None):
        """Extension: an allowed-token bitmask (int32 [B, n_words]: a TokenHealer's `mask`, DeviceStreamingDecoder.allowed_mask(), or
        xgrammar's) applied to logits [B, V] float32 / float16 / bfloat16 IN PLACE on the GPU, one launch
        (splintr_amd.device.mask_apply_device): -inf where a bit is 0, every other element untouched.  live uint8 [B]: rows with 0 are
        skipped.  Returns logits."""
        from . import device as dv
        return dv.mask_apply_device(self, logits, mask, live=live)

    def heal(self, texts_or_ids, *, max_back: int = 1, auto: bool = True, min_keep: int = 0, n_words: Optional[int] = None):
        """The one-call convenience for a list of prompts (str: encoded here; or lists of ids): -> (the trimmed ids, list[list[int]] --
        what to feed the model --, the TokenHealer whose mask constrains the first steps).  Synchronises once, for the trimmed lengths."""
        import torch
        from . import device as dv
        prompts = list(texts_or_ids)
        if prompts and all(isinstance(p, str) for p in prompts):
            prompts = self.encode_batch(prompts)
        prompts = [list(p) for p in prompts]
        healer = dv.TokenHealer(self, len(prompts), n_words=n_words, max_back=max_back, auto=auto)
        if not prompts:
            return [], healer
        L = max(1, max(len(p) for p in prompts))
        rows = torch.zeros((len(prompts), L), dtype=torch.int64)
        for i, p in enumerate(prompts):
            rows[i, :len(p)] = torch.tensor(p, dtype=torch.int64)
        dev = healer.mask.device
        n_back = healer.begin(rows.to(dev), torch.tensor([len(p) for p in prompts], dtype=torch.int32, device=dev), min_keep=min_keep)
        return [p[:len(p) - k] for p, k in zip(prompts, n_back.tolist())], healer

    # ------------------------------------------------------------------ cheap surface
    @property
    def vocab_size(self) -> int:
        """src/python/bindings.rs:382-385 -> src/core/tokenizer.rs:964-972."""
        return int(_ffi.lib().spl_vocab_size(self._h))

    @property
    def cache_len(self) -> int:
        """Tokenizer::cache_len (src/core/tokenizer.rs:1002-1005; bindings.rs:438-440).  The reference's LRU of encoded chunks is, on the GPU
        path, the chunk memo (csrc/spl_k_memo.h): result-transparent there and here.  The memo is filled BETWEEN launches, once the tiles have
        logged enough chunks it did not hold -- so unlike the reference's cache it may still be empty after one short text."""
        import ctypes
        out = (ctypes.c_uint64 * 4)()
        L = _ffi.lib()
        L.spl_memo_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        if L.spl_memo_stats(self.handle, out) != 0:
            raise RuntimeError(_ffi.last_error())
        return int(out[1] + out[2])

    def clear_cache(self) -> None:
        """Tokenizer::clear_cache (src/core/tokenizer.rs:995-1000): the memo starts empty again."""
        if _ffi.lib().spl_set_option(self.handle, b"memo_clear", 1) != 0:
            raise RuntimeError(_ffi.last_error())

    @property
    def has_custom_pattern(self) -> bool:
        """Extension: True when the split pattern is not one of the three the GPU scanner implements (its split then
        runs as a matcher program -- on the GPU, or on the host cores for what the device matcher gives up on --, and no context-free cut position is
        known for it: splintr_amd.distributed keeps such a tokenizer's documents whole)."""
        return self._pattern not in _PATTERN_ID

    def pcre2(self, use_pcre2: bool = True) -> "Tokenizer":
        """Backend switches (src/python/bindings.rs:207-242) select between regex engines that
        the reference's tests require to agree; here both map to the one scanner."""
        return self

    def jit(self, use_jit: bool = True) -> "Tokenizer":
        return self

    def __repr__(self) -> str:
        return f"Tokenizer(vocab_size={self.vocab_size})"

    # ------------------------------------------------------------------ backend hooks (bench / tests)
    @property
    def handle(self) -> int:
        return self._h
