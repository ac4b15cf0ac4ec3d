"""WordPiece mode (BERT-family vocabularies): the normalisation table the device reads, its host mirror, and vocab.txt parsing.

The semantics are those of Hugging Face's BertNormalizer -> BertPreTokenizer -> WordPiece, restated as a function of single code points
(DESIGN.md 4.24): every input code point maps to at most three output code points, each PLAIN, ISOLATED (a word of its own) or SPACE.
build_norm_table writes that function down for all of Unicode, from the running interpreter's unicodedata, as the two-stage table
csrc/spl_k_wp.h looks up; normalize_words applies the very same table on the host.
"""
import functools
import struct
import unicodedata
from typing import List, Optional, Tuple

PLAIN, ISOLATED, SPACE = 0, 1, 2
NORM_SHIFT = 7                       # code points per stage-2 block: 128
# Rust's char::is_whitespace (the White_Space property)
_WHITE_SPACE = frozenset([0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000, *range(0x09, 0x0E), *range(0x2000, 0x200B)])
# BERT's _is_chinese_char
_CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
        (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def _is_punct(c: int) -> bool:
    return 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126 or unicodedata.category(chr(c)).startswith("P")


def map_code_point(c: int, lowercase: bool, strip_accents: bool, handle_chinese_chars: bool, clean_text: bool) -> Tuple[Tuple[int, int], ...]:
    """What one input code point becomes: () if it is dropped, ((0x20, SPACE),), or up to three (code point, PLAIN | ISOLATED)."""
    if c in (0x09, 0x0A, 0x0D):
        return ((0x20, SPACE),)
    cat = unicodedata.category(chr(c))
    if cat == "Cs" or (clean_text and (c == 0 or c == 0xFFFD or cat in ("Cc", "Cf", "Cn", "Co"))):
        return ()
    if c in _WHITE_SPACE:
        return ((0x20, SPACE),)
    if handle_chinese_chars and any(lo <= c <= hi for lo, hi in _CJK):
        return ((c, ISOLATED),)
    s = chr(c)
    if strip_accents:
        s = "".join(x for x in unicodedata.normalize("NFD", s) if unicodedata.category(x) != "Mn")
    if lowercase:
        s = "".join(x.lower() for x in s)
    return tuple((ord(x), ISOLATED if _is_punct(ord(x)) else PLAIN) for x in s)


def build_norm_table(lowercase: bool = True, strip_accents: Optional[bool] = None, handle_chinese_chars: bool = True,
                     clean_text: bool = True) -> bytes:
    """The table as spl_opts.norm_table takes it.  Header: "SPLN", version 1, shift, stage-1 entries, stage-2 entries, words of the
    expansion list, two reserved words; then stage 1 (uint16 block numbers), stage 2 (uint32 per code point of a block) and the expansion
    list (uint32).  A stage-2 entry: bits 0-1 the number of output code points n; n == 1: bit 2 ISOLATED, bit 3 SPACE, bits 8-28 the
    output code point minus the input one modulo 2^21 (blocks of unchanged code points are all alike); n >= 2: bits 8-28 the index of n
    words of the expansion list, each a code point with bit 21 set if it is ISOLATED."""
    return _build(bool(lowercase), bool(lowercase if strip_accents is None else strip_accents), bool(handle_chinese_chars), bool(clean_text))


@functools.lru_cache(maxsize=None)
def _build(lowercase: bool, strip: bool, handle_chinese_chars: bool, clean_text: bool) -> bytes:
    blocks, stage1, stage2, multi, multi_at = {}, [], [], [], {}
    per = 1 << NORM_SHIFT
    for b0 in range(0, 0x110000, per):
        ent = []
        for c in range(b0, b0 + per):
            out = map_code_point(c, lowercase, strip, handle_chinese_chars, clean_text)
            n_in = len(chr(c).encode("utf-8", "surrogatepass"))
            n_out = sum(len(chr(o).encode("utf-8")) for o, _ in out)
            # the three facts the device relies on: the staging of a tile, the factor 3 of the workspace, "n_bytes ids always suffice"
            assert len(out) <= 3, f"U+{c:04X} maps to more than 3 code points"
            assert n_out - n_in <= 8 and n_out <= 3 * n_in, f"U+{c:04X} grows by more than 8 bytes or beyond three times its length"
            assert len(out) <= n_in, f"U+{c:04X} yields more code points than it has bytes"
            assert all(k == SPACE or o not in _WHITE_SPACE for o, k in out), f"U+{c:04X} maps to whitespace"
            if len(out) == 0:
                ent.append(0)
            elif len(out) == 1:
                o, k = out[0]
                ent.append(1 | (4 if k == ISOLATED else 0) | (8 if k == SPACE else 0) | (((o - c) & 0x1FFFFF) << 8))
            else:
                if out not in multi_at:
                    multi_at[out] = len(multi)
                    multi.extend(o | ((1 << 21) if k == ISOLATED else 0) for o, k in out)
                ent.append(len(out) | (multi_at[out] << 8))
        key = tuple(ent)
        if key not in blocks:
            blocks[key] = len(blocks)
            stage2.extend(ent)
        stage1.append(blocks[key])
    assert len(blocks) < 65536 and len(multi) < (1 << 21)
    head = struct.pack("<4s7I", b"SPLN", 1, NORM_SHIFT, len(stage1), len(stage2), len(multi), 0, 0)
    s1 = struct.pack(f"<{len(stage1)}H", *stage1)
    return head + s1 + b"\0" * (-len(s1) % 4) + struct.pack(f"<{len(stage2)}I", *stage2) + struct.pack(f"<{len(multi)}I", *multi)


def table_lookup(table: bytes, c: int) -> Tuple[Tuple[int, int], ...]:
    """One code point through the table, as the device kernel reads it."""
    _, _, shift, n1, n2, _, _, _ = struct.unpack_from("<4s7I", table, 0)
    at2 = 32 + 2 * n1 + (-2 * n1 % 4)
    blk, = struct.unpack_from("<H", table, 32 + 2 * (c >> shift))
    e, = struct.unpack_from("<I", table, at2 + 4 * ((blk << shift) | (c & ((1 << shift) - 1))))
    n = e & 3
    if n == 0:
        return ()
    if n == 1:
        return ((0x20, SPACE),) if e & 8 else (((c + (e >> 8)) & 0x1FFFFF, ISOLATED if e & 4 else PLAIN),)
    ws = struct.unpack_from(f"<{n}I", table, at2 + 4 * n2 + 4 * (e >> 8))
    return tuple((w & 0x1FFFFF, ISOLATED if w >> 21 else PLAIN) for w in ws)


def normalize_words(text: str, lowercase: bool = True, strip_accents: Optional[bool] = None, handle_chinese_chars: bool = True,
                    clean_text: bool = True) -> List[str]:
    """The words WordPiece matches, from the table: maximal runs of PLAIN output code points, and every ISOLATED one by itself."""
    table = build_norm_table(lowercase, strip_accents, handle_chinese_chars, clean_text)
    words, cur = [], []
    for ch in text:
        for o, k in table_lookup(table, ord(ch)):
            if k != PLAIN and cur:
                words.append("".join(cur))
                cur = []
            if k == PLAIN:
                cur.append(chr(o))
            elif k == ISOLATED:
                words.append(chr(o))
    if cur:
        words.append("".join(cur))
    return words


def parse_vocab_txt(data: bytes) -> List[bytes]:
    """vocab.txt: one token per line, id = line number (a trailing carriage return is not part of the token).  ValueError, naming the
    mode, for what spl_create refuses as well: an empty line inside the file, a key of more than 255 bytes, a key listed twice."""
    lines = bytes(data).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    keys = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
    seen = set()
    for i, k in enumerate(keys):
        if not k:
            raise ValueError(f"WordPiece mode: vocab.txt line {i + 1} is empty")
        if len(k) > 255:
            raise ValueError(f"WordPiece mode: vocab.txt line {i + 1}: a key of more than 255 bytes")
        if k in seen:
            raise ValueError(f"WordPiece mode: vocab.txt line {i + 1}: the key is listed twice")
        seen.add(k)
    if not keys:
        raise ValueError("WordPiece mode: vocab.txt is empty")
    return keys
