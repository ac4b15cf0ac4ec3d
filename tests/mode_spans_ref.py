"""Where every token of WordPiece mode and Unigram mode lies in its document, in plain Python: the reference of
test_mode_spans_cpu.py and test_gpu_mode_spans.py.  It imports nothing from the product.  Every output character has a SOURCE, one input
character as a byte range; a token spans from the start of its first character's source to the end of its last's.  A document is bytes:
a byte of no well-formed character is a lone escape of one byte (dropped by WordPiece, a character no key equals for Unigram)."""
import unicodedata

from wordpiece_ref import CJK, WHITE_SPACE, is_punct

MARK = "▁"


def _chars(doc):
    out, p = [], 0
    for ch in doc.decode("utf-8", "surrogateescape"):
        n = 1 if 0xDC80 <= ord(ch) <= 0xDCFF else len(ch.encode())
        out.append((ch, p, p + n))
        p += n
    return out


def wordpiece_spans(doc, vocab, unk_id, max_chars=100, prefix="##", lowercase=True, strip_accents=None, handle_chinese_chars=True,
                    clean_text=True):
    """(ids, byte spans).  Dropped code points, spaces and ill-formed bytes are the source of nothing; the prefix has no source."""
    strip = lowercase if strip_accents is None else strip_accents
    words, cur = [], []
    for ch, s, e in _chars(doc):
        c, cat = ord(ch), unicodedata.category(ch)
        if 0xDC80 <= c <= 0xDCFF or (ch not in "\t\n\r" and clean_text and (c == 0 or c == 0xFFFD or cat in ("Cc", "Cf", "Cn", "Co"))):
            continue
        if ch in "\t\n\r" or c in WHITE_SPACE:
            out = [None]
        elif handle_chinese_chars and any(lo <= c <= hi for lo, hi in CJK):
            out = [(ch, True)]
        else:
            t = "".join(x for x in unicodedata.normalize("NFD", ch) if unicodedata.category(x) != "Mn") if strip else ch
            out = [(x, is_punct(x)) for x in (t.lower() if lowercase else t)]
        for o in out:                                 # None a space, (x, True) an isolated character, (x, False) a plain one
            if o and not o[1]:
                cur.append((o[0], s, e))
                continue
            words += [cur] if cur else []
            cur = []
            words += [[(o[0], s, e)]] if o else []
    ids, spans = [], []
    for w in words + ([cur] if cur else []):
        text, pieces, i = "".join(x for x, _, _ in w), [], 0
        while i < len(w) <= max_chars:
            j = len(w)
            while j > i and ((prefix if i else "") + text[i:j]) not in vocab:
                j -= 1
            if j == i:
                break
            pieces.append((vocab[(prefix if i else "") + text[i:j]], w[i][1], w[j - 1][2]))
            i = j
        if i < len(w):                                # a position the loop reaches without a key, or a word over the limit: unk, the whole word
            pieces = [(unk_id, w[0][1], w[-1][2])]
        ids += [p[0] for p in pieces]
        spans += [(p[1], p[2]) for p in pieces]
    return ids, spans


def unigram_spans(doc, pieces, unk_id, prepend="always"):
    """(ids, byte spans).  A space matched as the marker is its one byte; the prepended marker's source is the document's first character;
    a fused run of unk spans from its first source to its last."""
    vocab, scores = {p: i for i, (p, _) in enumerate(pieces)}, [s for _, s in pieces]
    unk_score, longest = min(scores) - 10.0, max(map(len, vocab))
    chars = [(MARK if ch == " " else ch, s, e) for ch, s, e in _chars(doc)]
    if prepend == "always" and chars and chars[0][0] != MARK:
        chars.insert(0, (MARK,) + chars[0][1:])
    ids, spans, b = [], [], 0
    while b < len(chars):
        n = next((k for k in range(1, len(chars) - b) if chars[b + k][0] == MARK), len(chars) - b)
        w, word = chars[b:b + n], "".join(c[0] for c in chars[b:b + n])
        b += n
        best, back = [0.0] + [None] * n, [None] * (n + 1)
        for s in range(n):
            cands = [(e, vocab[word[s:e]]) for e in range(s + 1, min(n, s + longest) + 1) if word[s:e] in vocab]
            if not any(e == s + 1 for e, _ in cands):
                cands.append((s + 1, unk_id))         # (proposed last, at min_score - 10)
            for e, tid in cands:
                v = best[s] + (unk_score if tid == unk_id and word[s:e] not in vocab else scores[tid])
                if best[e] is None or v > best[e]:
                    best[e], back[e] = v, (s, tid)
        path, e = [], n
        while e:
            s, tid = back[e]
            path.append((tid, w[s][1], w[e - 1][2]))
            e = s
        prev_unk = False                              # (a run does not reach over a word's end)
        for tid, s, e in reversed(path):
            if tid == unk_id and prev_unk:
                spans[-1] = (spans[-1][0], e)
            else:
                ids.append(tid)
                spans.append((s, e))
            prev_unk = tid == unk_id
    return ids, spans


def to_chars(doc, spans):
    """Byte offsets to character offsets: offset p becomes the number of bytes b with (b & 0xC0) != 0x80 in doc[:p]."""
    pre = [0]
    for x in doc:
        pre.append(pre[-1] + ((x & 0xC0) != 0x80))
    return [(pre[a], pre[b]) for a, b in spans]
