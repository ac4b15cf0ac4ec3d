"""splintr_amd.nest.json_table against Python's own parser: json.loads(data.decode("utf-8"), parse_constant=<raises>) -- RFC 8259 with NaN
and Infinity refused; any ValueError, a decode error included, counts as a refusal.  Exhaustive over short byte strings, a seeded
generator of documents and their one-byte edits, the whitespace modes, the depth limit, shortest_completion, and the pinned state
counts."""
import itertools
import json
import random

import pytest

from splintr_amd import nest


def _refuse(name):
    raise ValueError(name)


def oracle(data: bytes) -> bool:
    try:
        json.loads(data.decode("utf-8"), parse_constant=_refuse)
        return True
    except (ValueError, RecursionError):
        return False


@pytest.fixture(scope="module")
def table():
    return nest.json_table()


ALPHABET = b'{}[]",:01- \\e.'                                         # both bracket pairs, the quote, , : 0 1 - space backslash, and e .


@pytest.fixture(scope="module")
def sweep(table):
    """every byte string of length <= 5 over ALPHABET that the "json" table accepts"""
    return [bytes(t) for n in range(6) for t in itertools.product(ALPHABET, repeat=n) if table.matches(bytes(t))]


def test_oracle_gives_the_answers_the_table_is_held_to():
    for data in (b"\xef\xbb\xbf1", b"NaN", b"Infinity", b"-Infinity", b"1.", b"01", b"-", b"[1,]", b'"\x01"', b'"\t"', b"\x0c1", b'"\xed\xa0\x80"',
                 b'"\xc0\x80"', b'"\\x"', b"", b" "):
        assert not oracle(data), data
    for data in (b"-0", b"1e5", b" 1 ", b'"\\ud800"', b'"\x7f"', b'{"a":1,"a":2}', b"[" * 70 + b"]" * 70):
        assert oracle(data), data


def test_named_inputs(table):
    for data in (b"\xef\xbb\xbf1", b"NaN", b"Infinity", b"-Infinity", b"1.", b"01", b"-", b"[1,]", b'"\x01"', b'"\t"', b"\x0c1", b'"\xed\xa0\x80"',
                 b'"\xc0\x80"', b'"\\x"', b"", b" ", b'"\xf4\x90\x80\x80"', b'"\xe0\x80\x80"', b'"\xf0\x80\x80\x80"', b'"\xc2"', b'"\x80"', b'"\\u12g4"',
                 b"1e", b"1e+", b"+1", b".5", b"tru", b"nul", b"truee", b"[1 2]", b'{"a" 1}', b'{"a":}', b"{1:2}", b'{"a":1,}', b"[}", b"]", b"1 2"):
        assert not table.matches(data) and not oracle(data), data
    for data in (b"-0", b"1e5", b" 1 ", b'"\\ud800"', b'"\x7f"', b'{"a":1,"a":2}', b"[" * 64 + b"]" * 64, b"0.5E-10", b"true", b" null\n", b"\tfalse\r",
                 b'"\xf4\x8f\xbf\xbf\xc2\x80\xe0\xa0\x80\xed\x9f\xbf\xee\x80\x80\xf0\x90\x80\x80"', b'"\\"\\\\\\/\\b\\f\\n\\r\\t\\uAbCd"', b"[ ]", b"{ }",
                 b'{ "a" : [ 1 , { } ] , "b" : "x" }', b"-1.5e+3", b"[[],[[]],{}]"):
        assert table.matches(data) and oracle(data), data
    assert not table.matches(b"[" * 70 + b"]" * 70)                            # (64 levels are the most a stack holds)


def test_exhaustive_short_strings(table, sweep):
    assert len(ALPHABET) >= 12
    accepted = set(sweep)
    n = 0
    for k in range(6):
        for t in itertools.product(ALPHABET, repeat=k):
            data = bytes(t)
            assert (data in accepted) == oracle(data), data
            n += 1
    assert n == sum(len(ALPHABET) ** k for k in range(6)) and len(accepted) > 1000


def gen_value(rng, depth):
    r = rng.random()
    if depth > 0 and r < 0.25:
        return [gen_value(rng, depth - 1) for _ in range(rng.randrange(4))]
    if depth > 0 and r < 0.5:
        return {gen_string(rng): gen_value(rng, depth - 1) for _ in range(rng.randrange(4))}
    if r < 0.6:
        return gen_string(rng)
    if r < 0.7:
        return rng.choice([True, False, None])
    if r < 0.85:
        return rng.choice([0, -1, 7, 10 ** 12, -305])
    return rng.choice([0.5, -1e-7, 3.25e20, -0.0, 12.75])


def gen_string(rng):
    pool = ["a", "Z", " ", '"', "\\", "\n", "\t", "\x7f", "\x1f", "é", "ß", "€", "語", "\U0001F30D", "ࠀ", "￿", "/", "\x00"]
    return "".join(rng.choice(pool) for _ in range(rng.randrange(6)))


def gen_document(rng):
    v = gen_value(rng, 8)
    for _ in range(rng.randrange(9)):                                  # nesting to depth 8
        v = [v] if rng.random() < 0.5 else {gen_string(rng): v}
    style = rng.randrange(4)
    if style == 0:
        return json.dumps(v, ensure_ascii=False).encode("utf-8")
    if style == 1:
        return json.dumps(v, ensure_ascii=True, separators=(",", ":")).encode("utf-8")
    if style == 2:
        return json.dumps(v, ensure_ascii=False, indent=rng.choice([1, "\t"])).encode("utf-8")
    return b" \r\n" + json.dumps(v, ensure_ascii=False, separators=(" ,\t", "\n: ")).encode("utf-8") + b"\t "


def test_generated_documents_and_one_byte_edits(table):
    rng = random.Random(8259)
    docs = [gen_document(rng) for _ in range(500)]
    assert max(d.count(b"[") + d.count(b"{") for d in docs) >= 8 and any(b"\xf0\x9f" in d for d in docs)
    for d in docs:
        assert oracle(d) and table.matches(d), d
    refused = 0
    for d in docs:
        at = rng.randrange(len(d))
        kind = rng.randrange(3)
        x = bytes([rng.choice(b'{}[]",:0-\\ e\x01\x80\xc0\xff\n') if rng.random() < 0.7 else rng.randrange(256)])
        e = d[:at] + x + d[at + 1:] if kind == 0 else (d[:at] + d[at + 1:] if kind == 1 else d[:at] + x + d[at:])
        want = oracle(e)
        assert table.matches(e) == want, e
        refused += not want
    assert 100 < refused < 500


@pytest.mark.parametrize("ws, separators", [("compact", (", ", ": ")), ("compact", (",", ":")), ("none", (",", ":"))])
def test_compact_and_none(ws, separators, sweep):
    t = nest.json_table(ws=ws)
    rng = random.Random(5)
    for _ in range(200):
        v = gen_value(rng, 4)
        d = json.dumps(v, ensure_ascii=False, separators=separators).encode("utf-8")
        assert t.matches(d) and oracle(d), d
        # a whitespace byte at a structural position is refused (inside a string it is part of the string)
        spots = [i for i in range(len(d) + 1) if _structural(d, i)]
        i = rng.choice(spots)
        for x in b" \t\n\r":
            e = d[:i] + bytes([x]) + d[i:]
            allowed_one = ws == "compact" and x == 0x20 and i > 0 and d[i - 1:i] in (b",", b":") and d[i:i + 1] != b" " and _structural(d, i - 1)
            assert t.matches(e) == allowed_one, (e, i)
    # everything the mode accepts in the exhaustive sweep the "json" mode accepts (and with it the oracle); what it refuses has whitespace
    mine = {bytes(s) for n in range(6) for s in itertools.product(ALPHABET, repeat=n) if t.matches(bytes(s))}
    assert mine <= set(sweep) and all(b" " in s for s in set(sweep) - mine) and len(mine) > 500
    assert t.matches(b"[0, 1]") == t.matches(b'{"a": 0}') == (ws == "compact") and b"[0,1]" in mine
    assert not any(t.matches(x) for x in (b"[0 ,1]", b" 1", b"1 ", b"[0,  1]", b"[ 0]", b"[0 ]", b'{"a" :0}', b'{ "a":0}', b"[0,\t1]"))


def _structural(d, i):
    """is position i of the document d outside every string (an insertion there is not inside a string's quotes)"""
    inside = esc = False
    for x in d[:i]:
        if inside:
            if esc:
                esc = False
            elif x == 0x5C:
                esc = True
            elif x == 0x22:
                inside = False
        elif x == 0x22:
            inside = True
    return not inside


def test_depth(table):
    for d in (1, 2, 15, 16, 17, 63, 64):
        assert table.matches(b"[" * d + b"]" * d, max_depth=d) and not table.matches(b"[" * (d + 1) + b"]" * (d + 1), max_depth=d)
        doc = b'{"k":' * d + b"0" + b"}" * d
        assert table.matches(doc, max_depth=d) and not table.matches(b"[" + doc + b"]", max_depth=d)
    assert table.matches(b"[" * 64 + b"]" * 64) and not table.matches(b"[" * 65 + b"]" * 65)


def test_shortest_completion_of_reachable_configurations(table):
    rng = random.Random(31)
    docs = [gen_document(rng) for _ in range(200)]
    seen = set()
    for d in docs:
        cut = d[:rng.randrange(len(d) + 1)]
        at = table.walk(table.start, (), cut)
        assert at is not None, cut
        for k in range(len(cut) + 1) if len(cut) < 40 else (len(cut),):         # every configuration on the way of a short prefix
            q, stack = table.walk(table.start, (), cut[:k])
            tail = table.shortest_completion(q, stack)
            assert tail is not None and oracle(cut[:k] + tail), (cut[:k], tail)
            seen.add((q, len(stack)))
    assert len({q for q, _ in seen}) > 60 and max(n for _, n in seen) >= 8
    q, stack = table.walk(table.start, (), b'{"a": [1, {"b": "x\\')
    assert table.shortest_completion(q, stack) == b'""}]}'
    assert table.shortest_completion(table.start, ()) == b"0" and nest.json_table("object").shortest_completion(0, ()) == b"{}"


def test_top_and_state_counts():
    obj, arr = nest.json_table("object"), nest.json_table("array")
    for data in (b"1", b'"a"', b"true", b"null", b"[]", b"[{}]", b" [1]"):
        assert not obj.matches(data), data
    for data in (b"{}", b' {"a":[1,{"b":null}]} ', b'{"a":1}'):
        assert obj.matches(data) and not arr.matches(data), data
    assert arr.matches(b"[1,{}]") and arr.matches(b" [ ] ") and not arr.matches(b"1") and not arr.matches(b"{}")
    counts = {(top, ws): nest.json_table(top, ws).n_states for top in ("value", "object", "array") for ws in ("json", "compact", "none")}
    assert counts == {("value", "json"): 116, ("value", "compact"): 119, ("value", "none"): 116,
                      ("object", "json"): 85, ("object", "compact"): 88, ("object", "none"): 85,
                      ("array", "json"): 85, ("array", "compact"): 88, ("array", "none"): 85}
    for t in (obj, arr, nest.json_table()):
        assert t.n_ret == 1 and t.start == 0 and int(t.op.astype(bool).sum()) > 0
        pushes = {int(o) & 15 for o in t.op.reshape(-1) if int(o) & 0xF0 == nest.PUSH}
        assert pushes == {nest.SYM_TOP, nest.SYM_MEMBER, nest.SYM_ELEMENT}
    with pytest.raises(ValueError, match="top must be"):
        nest.json_table("number")
    with pytest.raises(ValueError, match="ws must be"):
        nest.json_table(ws="any")
