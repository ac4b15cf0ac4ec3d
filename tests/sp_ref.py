"""SentencePiece mode as the reference runs it: a plain restatement of Tokenizer::encode's SentencePiece branch (src/core/tokenizer.rs:737-795)
and of encode_with_special (:843-874), with the pending counter kept literally.  The chunks of [^\\s]+|\\s+ come from an explicit
whitespace set -- PCRE2 10.39's UCP \\s -- and every byte string the loop hands to encode_bytes_with_cache is one `piece`: the ids are
byte_pair_encode of the pieces, the rewritten text is their concatenation, the chunk starts are where they begin."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.pyoracle import byte_pair_encode  # noqa: E402

WS = set([0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]) | set(range(0x09, 0x0E)) | set(range(0x2000, 0x200B))
MARK = "▁".encode()


def chunks(text: str):
    """find_iter of [^\\s]+|\\s+ as byte slices: maximal runs of whitespace characters and of everything else."""
    out, run, kind = [], "", None
    for ch in text:
        k = ord(ch) in WS
        if run and k != kind:
            out.append(run.encode())
            run = ""
        run, kind = run + ch, k
    if run:
        out.append(run.encode())
    return out


def pieces(text: str):
    """tokenizer.rs:743-793: what the loop encodes, piece by piece."""
    out, pending = [], 0
    for sl in chunks(text):
        if sl[0:1] in (b" ", b"\t", b"\n", b"\x0c", b"\r"):        # u8::is_ascii_whitespace
            for b in sl:
                if b == 0x20:
                    pending += 1
                else:
                    if pending > 0:
                        out.append(MARK * pending)
                        pending = 0
                    out.append(bytes([b]))
        else:
            out.append(MARK * pending + sl)
            pending = 0
    if pending > 0:
        out.append(MARK * pending)
    return out


_cache = {}                              # encode_bytes_with_cache: a piece is merged once per encoder (the oracle's merge loop is quadratic)


def _bpe(piece: bytes, encoder):
    key = (id(encoder), piece)
    if key not in _cache:
        _cache[key] = byte_pair_encode(piece, encoder)
    return _cache[key]


def encode(text: str, encoder):
    return [i for p in pieces(text) for i in _bpe(p, encoder)]


def split_special(text: str, special):
    """tokenizer.rs:851-871: the stretches between non-overlapping literal matches, leftmost first (the tests' literals neither
    contain nor chain into one another) -- ("text", str) and ("special", id) items in order."""
    out, last, i = [], 0, 0
    while i < len(text):
        hit = next((lit for lit in special if text.startswith(lit, i)), None)
        if hit is None:
            i += 1
            continue
        if i > last:
            out.append(("text", text[last:i]))
        out.append(("special", special[hit], hit))
        i = last = i + len(hit)
    if last < len(text):
        out.append(("text", text[last:]))
    return out


def encode_with_special(text: str, encoder, special):
    ids = []
    for item in split_special(text, special):
        ids += encode(item[1], encoder) if item[0] == "text" else [item[1]]
    return ids


def rewrite(texts, special=None):
    """The corpus as the merge path sees it: (rewritten bytes, sorted chunk-start positions, rewritten document offsets).  A literal
    is copied as it is and starts a chunk."""
    buf, starts, offs = b"", [], [0]
    for t in texts:
        items = split_special(t, special) if special else ([("text", t)] if t else [])
        for item in items:
            ps = pieces(item[1]) if item[0] == "text" else [item[2].encode()]
            for p in ps:
                starts.append(len(buf))
                buf += p
        offs.append(len(buf))
    return buf, starts, offs
