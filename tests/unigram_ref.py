"""Plain reference of Unigram mode: Hugging Face's pre_tokenizers.Metaspace -> models.Unigram.encode_optimized with
byte_fallback off and fuse_unk on, restated.  Imports nothing from the product.  A document is a str, or bytes: a byte that is not part
of a well-formed UTF-8 character is then a character by itself (a lone surrogate here), which no key equals."""
MARK = "▁"


def words(doc, prepend="always"):
    """The document's words: every space stands for U+2581, a word starts at the document's start and at every U+2581."""
    if isinstance(doc, bytes):
        doc = doc.decode("utf-8", "surrogateescape")
    doc = doc.replace(" ", MARK)
    if prepend == "always" and doc and not doc.startswith(MARK):
        doc = MARK + doc
    out = []
    for i, ch in enumerate(doc):
        if ch == MARK or i == 0:
            out.append("")
        out[-1] += ch
    return out


def encode_word(word, vocab, scores, unk_id):
    """The path of highest score: starts in ascending order, one f64 add per proposal, replaced only when strictly greater."""
    n, unk_score, longest = len(word), min(scores) - 10.0, max(map(len, vocab))
    best, back = [None] * (n + 1), [None] * (n + 1)
    best[0] = 0.0
    for s in range(n):
        single = False
        for e in range(s + 1, min(n, s + longest) + 1):
            tid = vocab.get(word[s:e])
            if tid is None:
                continue
            single |= e == s + 1
            if best[e] is None or best[s] + scores[tid] > best[e]:
                best[e], back[e] = best[s] + scores[tid], (s, tid)
        if not single and (best[s + 1] is None or best[s] + unk_score > best[s + 1]):
            best[s + 1], back[s + 1] = best[s] + unk_score, (s, unk_id)
    ids, e = [], n
    while e:
        e, tid = back[e]
        if not (tid == unk_id and ids and ids[-1] == unk_id):          # fuse_unk: a run of unk is one id
            ids.append(tid)
    return ids[::-1]


def encode(doc, pieces, unk_id, prepend="always"):
    """pieces: (piece, score) pairs, id = index."""
    vocab, scores = {p: i for i, (p, _) in enumerate(pieces)}, [s for _, s in pieces]
    return [t for w in words(doc, prepend) for t in encode_word(w, vocab, scores, unk_id)]
