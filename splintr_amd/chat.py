"""Chat templates as IDS: what wraps a message of each role, for `Tokenizer.encode_batch_chat` / `splintr_amd.device.chat_device`.

A template here is not a string to render and tokenize: it is, per role, the ids in front of a message (the header) and behind it (the
footer), the ids in front of a whole conversation (bos) and the generation prompt.  The messages are encoded by themselves and the device
joins header + content + footer per turn (csrc/spl_k_chat.h), so text inside a message can never become a control token.  For content that
begins with a letter or a digit the ids are exactly those of the rendered string encoded with special tokens; for other content (a
message that begins with "\\n\\n" under llama3) the ids differ at the seam, as for `encode_batch_pairs`.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence, Tuple

from . import _ffi


def _ids(name: str, ids, limit: int) -> Tuple[int, ...]:
    if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple)):
        raise ValueError(f"{name} must be a list or tuple of ids, not {type(ids).__name__}")
    if len(ids) > limit:
        raise ValueError(f"{name} holds {len(ids)} ids: at most {limit}")
    for v in ids:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < (1 << 32):
            raise ValueError(f"every id of {name} must be an integer that fits 32 bits, not {v!r}")
    return tuple(ids)


def message(m) -> Tuple[str, str]:
    """one message -- a {"role", "content"} dict or a (role, content) tuple -- as (role, content)"""
    if isinstance(m, Mapping):
        if "role" not in m or "content" not in m:
            raise ValueError("a message dict needs the keys 'role' and 'content'")
        role, content = m["role"], m["content"]
    elif isinstance(m, (tuple, list)) and len(m) == 2:
        role, content = m
    else:
        raise ValueError(f"a message must be a {{'role', 'content'}} dict or a (role, content) tuple, not {type(m).__name__}")
    if not isinstance(role, str) or not isinstance(content, str):
        raise ValueError("a message's role and content must be str")
    return role, content


class ChatTemplate:
    """roles: an ORDERED mapping name -> (header ids, footer ids); the position of a name is its role number on the device (at most 8
    roles, 16 header and 8 footer ids each).  bos: ids in front of every conversation (at most 8).  generation: the ids that ask for an
    answer, appended when add_generation_prompt is set (at most 16).  train: the roles whose message content carries labels;
    train_footer: whether the footer of such a message does too (the end-of-turn token a model must learn to emit).
    text: optional (per role (header string, footer string), bos string, generation string) for render()."""

    def __init__(self, roles: Mapping[str, Tuple[Sequence[int], Sequence[int]]], bos: Sequence[int] = (), generation: Sequence[int] = (),
                 train: Sequence[str] = ("assistant",), train_footer: bool = True, text=None):
        if not isinstance(roles, Mapping) or not 1 <= len(roles) <= _ffi.SPL_CHAT_MAX_ROLES:
            raise ValueError(f"roles must be a mapping of 1 .. {_ffi.SPL_CHAT_MAX_ROLES} names to (header ids, footer ids)")
        self.roles: Dict[str, Tuple[Tuple[int, ...], Tuple[int, ...]]] = {}
        for name, pair in roles.items():
            if not isinstance(name, str) or not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError("roles must map a name to a (header ids, footer ids) pair")
            self.roles[name] = (_ids(f"the header of {name!r}", pair[0], _ffi.SPL_CHAT_MAX_HEADER),
                                _ids(f"the footer of {name!r}", pair[1], _ffi.SPL_CHAT_MAX_FOOTER))
        self.role_number = {name: i for i, name in enumerate(self.roles)}
        self.bos = _ids("bos", tuple(bos), _ffi.SPL_CHAT_MAX_BOS)
        self.generation = _ids("generation", tuple(generation), _ffi.SPL_CHAT_MAX_GEN)
        if isinstance(train, str):
            raise ValueError("train must be a sequence of role names")
        for name in train:
            if name not in self.roles:
                raise ValueError(f"train names the role {name!r}, which the template does not have")
        self.train = tuple(train)
        self.train_footer = bool(train_footer)
        self._text = text

    # ------------------------------------------------------------------ what the device is told
    @property
    def train_content_mask(self) -> int:
        return sum(1 << self.role_number[name] for name in set(self.train))

    @property
    def train_footer_mask(self) -> int:
        return self.train_content_mask if self.train_footer else 0

    def role_of(self, name: str) -> int:
        if name not in self.role_number:
            raise ValueError(f"unknown role {name!r}: the template has {', '.join(self.roles)}")
        return self.role_number[name]

    # ------------------------------------------------------------------ the built-in formats
    @staticmethod
    def _special(tok, special_tokens: Optional[Mapping[str, int]], names: Sequence[str]) -> Dict[str, int]:
        table = special_tokens if special_tokens is not None else getattr(tok, "_special", None)
        if table is None:
            raise ValueError("the tokenizer has no special-token table: pass special_tokens=")
        for name in names:
            if name not in table:
                raise ValueError(f"the vocabulary has no special token {name}")
        return {name: int(table[name]) for name in names}

    @classmethod
    def chatml(cls, tok, special_tokens: Optional[Mapping[str, int]] = None, **kw) -> "ChatTemplate":
        """ChatML: <|im_start|>role\\n content <|im_end|>\\n per message, the generation prompt <|im_start|>assistant\\n; roles system,
        user, assistant, tool.  tok: anything with encode(str) -> ids; the two control ids come from its special-token table (or
        special_tokens)."""
        sp = cls._special(tok, special_tokens, ("<|im_start|>", "<|im_end|>"))
        names = ("system", "user", "assistant", "tool")
        footer = [sp["<|im_end|>"]] + list(tok.encode("\n"))
        roles = {r: ([sp["<|im_start|>"]] + list(tok.encode(r + "\n")), footer) for r in names}
        text = ({r: ("<|im_start|>" + r + "\n", "<|im_end|>\n") for r in names}, "", "<|im_start|>assistant\n")
        return cls(roles, (), roles["assistant"][0], text=text, **kw)

    @classmethod
    def llama3(cls, tok, special_tokens: Optional[Mapping[str, int]] = None, **kw) -> "ChatTemplate":
        """Llama 3: <|begin_of_text|> once, then <|start_header_id|>role<|end_header_id|>\\n\\n content <|eot_id|> per message; roles
        system, user, assistant, ipython."""
        sp = cls._special(tok, special_tokens, ("<|begin_of_text|>", "<|start_header_id|>", "<|end_header_id|>", "<|eot_id|>"))
        names = ("system", "user", "assistant", "ipython")
        roles = {r: ([sp["<|start_header_id|>"]] + list(tok.encode(r)) + [sp["<|end_header_id|>"]] + list(tok.encode("\n\n")), [sp["<|eot_id|>"]])
                 for r in names}
        text = ({r: ("<|start_header_id|>" + r + "<|end_header_id|>\n\n", "<|eot_id|>") for r in names}, "<|begin_of_text|>",
                "<|start_header_id|>assistant<|end_header_id|>\n\n")
        return cls(roles, (sp["<|begin_of_text|>"],), roles["assistant"][0], text=text, **kw)

    def render(self, conversation, add_generation_prompt: bool = False) -> str:
        """The string form of a conversation -- for documentation and tests only: the device never sees it."""
        if self._text is None:
            raise ValueError("this template was built from ids alone: it has no string form")
        per_role, bos, gen = self._text
        out = [bos]
        for m in conversation:
            role, content = message(m)
            self.role_of(role)
            out += [per_role[role][0], content, per_role[role][1]]
        if add_generation_prompt:
            out.append(gen)
        return "".join(out)
