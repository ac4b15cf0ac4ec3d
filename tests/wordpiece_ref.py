"""WordPiece mode in plain Python: whole strings in, ids out, from unicodedata and a dict.  The reference of
test_wordpiece_cpu.py and test_gpu_wordpiece.py; it imports nothing from the product."""
import unicodedata

WHITE_SPACE = {0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000, *range(0x09, 0x0E), *range(0x2000, 0x200B)}
CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
       (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def is_punct(ch):
    c = ord(ch)
    return 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126 or unicodedata.category(ch).startswith("P")


def words(text, lowercase=True, strip_accents=None, handle_chinese_chars=True, clean_text=True):
    """Steps 1 and 2: the words of one document (a str, or bytes whose ill-formed parts are dropped)."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "ignore")
    strip = lowercase if strip_accents is None else strip_accents
    out, cur = [], ""
    for ch in text:
        c, cat = ord(ch), unicodedata.category(ch)
        if ch in "\t\n\r":
            piece = [" "]
        elif clean_text and (c == 0 or c == 0xFFFD or cat in ("Cc", "Cf", "Cn", "Co")):
            continue
        elif c in WHITE_SPACE:
            piece = [" "]
        elif handle_chinese_chars and any(lo <= c <= hi for lo, hi in CJK):
            piece = [(ch,)]
        else:
            s = ch
            if strip:
                s = "".join(x for x in unicodedata.normalize("NFD", s) if unicodedata.category(x) != "Mn")
            if lowercase:
                s = "".join(x.lower() for x in s)
            piece = [(x,) if is_punct(x) else x for x in s]
        for p in piece:                               # " " a space, (x,) an isolated character, x a plain one
            if isinstance(p, str) and p != " ":
                cur += p
                continue
            if cur:
                out.append(cur)
                cur = ""
            if p != " ":
                out.append(p[0])
    return out + ([cur] if cur else [])


def encode_word(word, vocab, unk_id, max_chars=100, prefix="##"):
    """Step 3: greedy longest match first; a position the loop reaches without a match makes the whole word unk_id."""
    if len(word) > max_chars:
        return [unk_id]
    ids, s = [], 0
    while s < len(word):
        e = len(word)
        while e > s and ((prefix if s else "") + word[s:e]) not in vocab:
            e -= 1
        if e == s:
            return [unk_id]
        ids.append(vocab[(prefix if s else "") + word[s:e]])
        s = e
    return ids


def encode(text, vocab, unk_id, max_chars=100, prefix="##", **norm):
    return [i for w in words(text, **norm) for i in encode_word(w, vocab, unk_id, max_chars, prefix)]
