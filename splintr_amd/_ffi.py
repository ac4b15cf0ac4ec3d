"""ctypes binding of libsplintr_hip.so (include/splintr_hip.h).

The library is the product: if it is missing or cannot be loaded this module raises -- there is
no CPU fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPL_LIB_PATH: development override used to A/B kernel variants built with different -D flags
LIB_PATH = os.environ.get("SPL_LIB_PATH") or os.path.join(_HERE, "libsplintr_hip.so")

SPL_OK = 0
SPL_WITH_SPECIAL = 1
SPL_INTRA_DOC = 2
SPL_MAX_KERNELS = 16

# every symbol include/splintr_hip.h declares (tests/test_abi.py checks the header against this)
SYMBOLS = [
    "spl_last_error", "spl_device_count", "spl_create", "spl_add_special", "spl_vocab_size", "spl_destroy",
    "spl_reserve", "spl_encode_batch", "spl_result_tokens", "spl_result_offsets", "spl_result_n_tokens",
    "spl_result_n_docs", "spl_result_free", "spl_encode_batch_device", "spl_decode_batch", "spl_free",
    "spl_profile_enable", "spl_profile_reset", "spl_profile_read", "spl_kernel_name", "spl_last_queue_counts",
    "spl_debug_phases", "spl_debug_blocks", "spl_debug_rebase_offsets", "spl_gatherv_pack", "spl_gatherv_unpack", "spl_gatherv_unpack_group", "spl_encode_batch_device_packed",
    "spl_set_devices", "spl_n_devices", "spl_set_option", "spl_host_alloc", "spl_host_free",
    "spl_token_bytes", "spl_is_byte_level",
    "spl_comm_unique_id", "spl_comm_create", "spl_comm_destroy", "spl_comm_rank", "spl_comm_world",
    "spl_allgather_slabs", "spl_allgather_slabs_p2p", "spl_gatherv_unpack_at", "spl_allgatherv_csr", "spl_split_host", "spl_encode_chunks_device",
    "spl_split_device", "spl_device_split_fallbacks", "spl_small_path_calls", "spl_pick_stream", "spl_memo_stats", "spl_memo_seed_stats", "spl_debug_memo_entry",
    "spl_pad_device", "spl_pack_device", "spl_pair_device", "spl_chat_work_bytes", "spl_chat_device", "spl_seqpack_work_bytes", "spl_seqpack_device", "spl_window_work_bytes", "spl_window_device",
    "spl_decode_reserve_device", "spl_decode_batch_device", "spl_max_token_bytes", "spl_token_spans_device",
    "spl_stream_reserve_device", "spl_stream_decode_device",
    "spl_get_option", "spl_stop_reserve_device", "spl_stop_match_device",
    "spl_heal_reserve_device", "spl_heal_begin_device", "spl_heal_step_device",
    "spl_utf8_mask_reserve_device", "spl_utf8_mask_device", "spl_mask_apply_device",
    "spl_choice_reserve_device", "spl_choice_step_device",
    "spl_dfa_reserve_device", "spl_dfa_index_device", "spl_dfa_step_device", "spl_dfa_jump_index_device", "spl_dfa_jump_device",
    "spl_nest_reserve_device", "spl_nest_index_device", "spl_nest_step_device",
    "spl_dfa_draft_device", "spl_nest_draft_device",
]
SPL_PATTERN_CUSTOM = 3
SPL_OPT_BYTE_LEVEL = 1
SPL_COLLATE_I64, SPL_COLLATE_PAD_LEFT, SPL_COLLATE_KEEP_TAIL, SPL_COLLATE_BOS, SPL_COLLATE_EOS = 1, 2, 4, 8, 16
SPL_PAIR_MAX_FIXED, SPL_PAIR_KEEP_TAIL_A, SPL_PAIR_KEEP_TAIL_B = 32, 32, 64
SPL_PAIR_LONGEST_FIRST, SPL_PAIR_ONLY_FIRST, SPL_PAIR_ONLY_SECOND = 0, 1, 2
SPL_CHAT_DROP_OLDEST, SPL_CHAT_PIN_FIRST, SPL_CHAT_NO_ROLE = 32, 64, 255
SPL_CHAT_MAX_ROLES, SPL_CHAT_MAX_HEADER, SPL_CHAT_MAX_FOOTER, SPL_CHAT_MAX_BOS, SPL_CHAT_MAX_GEN = 8, 16, 8, 8, 16
SPL_SEQPACK_NEXT_FIT, SPL_SEQPACK_BEST_FIT_DECREASING, SPL_SEQPACK_MASK_FIRST, SPL_SEQPACK_BFD_MAX_ROW_LEN = 0, 1, 32, 32768
SPL_DECODE_I64, SPL_DECODE_PAD_LEFT, SPL_DECODE_SKIP_SPECIAL = 1, 2, 4
SPL_SPANS_I64 = 1
SPL_STREAM_REPLACE, SPL_STREAM_FINAL_ALL = 1, 2
SPL_STOP_SLOTS, SPL_STOP_MAX_LEN, SPL_STOP_TABLE_BYTES, SPL_STOP_STATE_WORDS = 64, 64, 64 * 64 + 64, 10
SPL_STOP_INCLUDE, SPL_STOP_FINAL_ALL = 1, 2
SPL_HEAL_AUTO, SPL_HEAL_KEEP_FREE, SPL_HEAL_I64, SPL_HEAL_PAD_LEFT = 1, 2, 4, 8
SPL_HEAL_STATE_WORDS, SPL_HEAL_MAX_PREFIX, SPL_HEAL_MAX_BACK = 9, 64, 8
SPL_UTF8_AND = 1
SPL_F32, SPL_F16, SPL_BF16 = 0, 1, 2
SPL_CHOICE_THEN_FREE, SPL_CHOICE_KEEP_FREE, SPL_CHOICE_I64 = 1, 2, 4
SPL_CHOICE_SLOTS, SPL_CHOICE_MAX_LEN, SPL_CHOICE_TABLE_BYTES, SPL_CHOICE_STATE_WORDS, SPL_CHOICE_MAX_END = 64, 64, 64 * 64 + 64, 2, 8
SPL_DFA_KEEP_FREE, SPL_DFA_I64 = 2, 4
SPL_DFA_DEAD, SPL_DFA_MAX_STATES, SPL_DFA_STATE_WORDS, SPL_DFA_MAX_END = 0xFFFF, 4096, 1, 8
SPL_DFA_JUMP_MAX_BYTES, SPL_DFA_JUMP_MAX_IDS = 64, 64
SPL_NEST_KEEP_FREE, SPL_NEST_I64, SPL_NEST_PUSH, SPL_NEST_POP = 2, 4, 0x10, 0x20
SPL_NEST_MAX_STATES, SPL_NEST_MAX_RET, SPL_NEST_MAX_DEPTH, SPL_NEST_STATE_WORDS, SPL_NEST_MAX_END = 4096, 4096, 64, 5, 8
SPL_DRAFT_MAX_NODES, SPL_DRAFT_PARENT_PER_SEQ = 64, 1
SPL_ECAPACITY = -3


def SPL_DFA_TABLE_BYTES(n_states: int) -> int:
    return n_states * 512 + n_states


def SPL_DFA_JUMP_INDEX_BYTES(n_states: int) -> int:
    return n_states * (64 * 4 + 1 + 1 + 64)


def SPL_DFA_INDEX_BYTES(n_states: int, n_words: int) -> int:
    return n_states * (((n_words + 3) & ~3) * 4 + 1)


def SPL_NEST_TABLE_BYTES(n_states: int, n_ret: int) -> int:
    return n_states * 769 + n_ret * 32


def SPL_NEST_INDEX_BYTES(n_states: int, n_words: int, dep_cap: int) -> int:
    return n_states * (((n_words + 3) & ~3) * 4 + 5) + 4 + dep_cap * 4


class SplOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("pattern", ctypes.c_int32), ("device", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("pattern_text", ctypes.c_char_p), ("pattern_len", ctypes.c_uint64)]

    def __init__(self, pattern=0, device=0, flags=0, pattern_text=None):
        super().__init__(ctypes.sizeof(SplOpts), pattern, device, flags, pattern_text, len(pattern_text) if pattern_text else 0)


class SplCollateOpts(ctypes.Structure):
    """spl_collate_opts (include/splintr_hip.h): what spl_pad_device / spl_pack_device are told about a row."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("row_len", ctypes.c_uint32),
                ("pad_id", ctypes.c_uint32), ("bos_id", ctypes.c_uint32), ("eos_id", ctypes.c_uint32)]

    def __init__(self, flags=0, row_len=0, pad_id=0, bos_id=0, eos_id=0):
        super().__init__(ctypes.sizeof(SplCollateOpts), flags, row_len, pad_id, bos_id, eos_id)


class SplPairOpts(ctypes.Structure):
    """spl_pair_opts (include/splintr_hip.h): what spl_pair_device is told about a row -- the three fixed segments are HOST values."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("row_len", ctypes.c_uint32), ("pad_id", ctypes.c_uint32),
                ("trunc", ctypes.c_uint32), ("n_prefix", ctypes.c_uint32), ("n_middle", ctypes.c_uint32), ("n_suffix", ctypes.c_uint32),
                ("prefix", ctypes.c_uint32 * 32), ("middle", ctypes.c_uint32 * 32), ("suffix", ctypes.c_uint32 * 32)]

    def __init__(self, flags=0, row_len=0, pad_id=0, trunc=0, prefix=(), middle=(), suffix=()):
        seg = ctypes.c_uint32 * 32
        super().__init__(ctypes.sizeof(SplPairOpts), flags, row_len, pad_id, trunc, len(prefix), len(middle), len(suffix),
                         seg(*prefix[:32]), seg(*middle[:32]), seg(*suffix[:32]))


class SplChatOpts(ctypes.Structure):
    """spl_chat_opts (include/splintr_hip.h): what spl_chat_device is told about a row and the template -- HOST values.  roles: one
    (header ids, footer ids) per role number; train_content / train_footer: bit masks over the role numbers."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("row_len", ctypes.c_uint32), ("pad_id", ctypes.c_uint32),
                ("ignore_id", ctypes.c_uint32), ("n_roles", ctypes.c_uint32), ("train_content", ctypes.c_uint32),
                ("train_footer", ctypes.c_uint32), ("n_bos", ctypes.c_uint32), ("n_gen", ctypes.c_uint32),
                ("n_header", ctypes.c_uint32 * 8), ("n_footer", ctypes.c_uint32 * 8), ("bos", ctypes.c_uint32 * 8), ("gen", ctypes.c_uint32 * 16),
                ("header", ctypes.c_uint32 * 16 * 8), ("footer", ctypes.c_uint32 * 8 * 8)]

    def __init__(self, flags=0, row_len=0, pad_id=0, ignore_id=0xFFFFFF9C, roles=(((), ()),), train_content=0, train_footer=0, bos=(), gen=()):
        roles = [(tuple(h), tuple(f)) for h, f in roles]
        super().__init__(ctypes.sizeof(SplChatOpts), flags, row_len, pad_id, ignore_id & 0xFFFFFFFF, len(roles), train_content, train_footer,
                         len(bos), len(gen))
        for r, (h, f) in enumerate(roles[:8]):
            self.n_header[r], self.n_footer[r] = len(h), len(f)
            for j, v in enumerate(h[:16]):
                self.header[r][j] = v
            for j, v in enumerate(f[:8]):
                self.footer[r][j] = v
        for j, v in enumerate(bos[:8]):
            self.bos[j] = v
        for j, v in enumerate(gen[:16]):
            self.gen[j] = v


class SplSeqpackOpts(ctypes.Structure):
    """spl_seqpack_opts (include/splintr_hip.h): the row, the strategy and what pads each output of spl_seqpack_device."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("strategy", ctypes.c_uint32), ("row_len", ctypes.c_uint32),
                ("pad_id", ctypes.c_uint32), ("ignore_id", ctypes.c_uint32), ("fill", ctypes.c_uint8 * 4)]

    def __init__(self, flags=0, strategy=0, row_len=0, pad_id=0, ignore_id=0xFFFFFF9C, fill=(0, 0, 0, 0)):
        super().__init__(ctypes.sizeof(SplSeqpackOpts), flags, strategy, row_len, pad_id, ignore_id & 0xFFFFFFFF, (ctypes.c_uint8 * 4)(*fill))


class SplSeqpackIn(ctypes.Structure):
    """spl_seqpack_in: the sequences -- rows + lengths, or a CSR -- and their companions, device addresses (None: not given)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_len", ctypes.c_uint32), ("n_seqs", ctypes.c_uint64), ("d_ids", ctypes.c_void_p),
                ("d_lengths", ctypes.c_void_p), ("d_off", ctypes.c_void_p), ("d_labels", ctypes.c_void_p), ("d_bytes", ctypes.c_void_p * 4)]

    def __init__(self, n_seqs=0, in_len=0, ids=None, lengths=None, off=None, labels=None, byte_arrays=(None,) * 4):
        super().__init__(ctypes.sizeof(SplSeqpackIn), in_len, n_seqs, ids, lengths, off, labels, (ctypes.c_void_p * 4)(*byte_arrays))


class SplSeqpackOut(ctypes.Structure):
    """spl_seqpack_out: where the outputs go, device addresses (None: not wanted)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("max_rows", ctypes.c_uint64), ("d_rows", ctypes.c_void_p),
                ("d_labels", ctypes.c_void_p), ("d_bytes", ctypes.c_void_p * 4), ("d_mask", ctypes.c_void_p), ("d_pos", ctypes.c_void_p),
                ("d_seq", ctypes.c_void_p), ("d_place", ctypes.c_void_p), ("d_fill", ctypes.c_void_p), ("d_cu", ctypes.c_void_p),
                ("d_n", ctypes.c_void_p), ("d_status", ctypes.c_void_p)]

    def __init__(self, max_rows=0, rows=None, labels=None, byte_arrays=(None,) * 4, mask=None, pos=None, seq=None, place=None, fill=None,
                 cu=None, n=None, status=None):
        super().__init__(ctypes.sizeof(SplSeqpackOut), 0, max_rows, rows, labels, (ctypes.c_void_p * 4)(*byte_arrays), mask, pos, seq, place,
                         fill, cu, n, status)


class SplDecodeOpts(ctypes.Structure):
    """spl_decode_opts (include/splintr_hip.h): flags and the mode of spl_decode_batch_device (row_len 0: CSR, > 0: rows)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("row_len", ctypes.c_uint32)]

    def __init__(self, flags=0, row_len=0):
        super().__init__(ctypes.sizeof(SplDecodeOpts), flags, row_len)


class SplHealOpts(ctypes.Structure):
    """spl_heal_opts (include/splintr_hip.h): flags, the words of a mask row, and what a begin may take off a prompt."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("max_back", ctypes.c_uint32),
                ("min_keep", ctypes.c_uint32)]

    def __init__(self, flags=0, n_words=0, max_back=0, min_keep=0):
        super().__init__(ctypes.sizeof(SplHealOpts), flags, n_words, max_back, min_keep)


class SplHealIn(ctypes.Structure):
    """spl_heal_in: the rows of ids, their lengths and (step) the state rows, device addresses (None: not given)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("row_len", ctypes.c_uint32), ("n_seqs", ctypes.c_uint64), ("d_ids", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_state_in", ctypes.c_void_p)]

    def __init__(self, n_seqs=0, row_len=0, ids=None, lengths=None, state=None):
        super().__init__(ctypes.sizeof(SplHealIn), row_len, n_seqs, ids, lengths, state)


class SplHealOut(ctypes.Structure):
    """spl_heal_out: where the outputs go, device addresses (None: not wanted)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("d_state_out", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("d_live", ctypes.c_void_p), ("d_n", ctypes.c_void_p), ("d_n_back", ctypes.c_void_p)]

    def __init__(self, state=None, mask=None, live=None, n=None, n_back=None):
        super().__init__(ctypes.sizeof(SplHealOut), 0, state, mask, live, n, n_back)


class SplMaskApply(ctypes.Structure):
    """spl_mask_apply (include/splintr_hip.h): the logits, the mask rows and the live bytes of spl_mask_apply_device, device addresses."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("dtype", ctypes.c_uint32), ("d_logits", ctypes.c_void_p), ("n_rows", ctypes.c_uint64),
                ("n_cols", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("row_stride", ctypes.c_uint64), ("mask_stride", ctypes.c_uint64),
                ("d_mask", ctypes.c_void_p), ("d_live", ctypes.c_void_p)]

    def __init__(self, dtype=0, logits=None, n_rows=0, n_cols=0, n_words=0, row_stride=0, mask_stride=0, mask=None, live=None):
        super().__init__(ctypes.sizeof(SplMaskApply), dtype, logits, n_rows, n_cols, n_words, row_stride, mask_stride, mask, live)


class SplChoiceOpts(ctypes.Structure):
    """spl_choice_opts (include/splintr_hip.h): flags, the words of a mask row and the END ids, by value."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("n_end", ctypes.c_uint32),
                ("end_ids", ctypes.c_uint32 * 8)]

    def __init__(self, flags=0, n_words=0, end_ids=()):
        end_ids = tuple(end_ids)
        super().__init__(ctypes.sizeof(SplChoiceOpts), flags, n_words, len(end_ids), (ctypes.c_uint32 * 8)(*end_ids[:8]))


class SplChoiceIn(ctypes.Structure):
    """spl_choice_in: the rows of ids, their lengths, the state rows and the choice table, device addresses (None: not given)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("row_len", ctypes.c_uint32), ("n_seqs", ctypes.c_uint64), ("d_ids", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_state_in", ctypes.c_void_p), ("d_table", ctypes.c_void_p)]

    def __init__(self, n_seqs=0, row_len=0, ids=None, lengths=None, state=None, table=None):
        super().__init__(ctypes.sizeof(SplChoiceIn), row_len, n_seqs, ids, lengths, state, table)


class SplChoiceOut(ctypes.Structure):
    """spl_choice_out: where the outputs go, device addresses (None: not wanted)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("d_state_out", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("d_live", ctypes.c_void_p)]

    def __init__(self, state=None, mask=None, live=None):
        super().__init__(ctypes.sizeof(SplChoiceOut), 0, state, mask, live)


class SplDfaOpts(ctypes.Structure):
    """spl_dfa_opts (include/splintr_hip.h): flags, the words of a mask row and the END ids, by value."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("n_end", ctypes.c_uint32),
                ("end_ids", ctypes.c_uint32 * 8)]

    def __init__(self, flags=0, n_words=0, end_ids=()):
        end_ids = tuple(end_ids)
        super().__init__(ctypes.sizeof(SplDfaOpts), flags, n_words, len(end_ids), (ctypes.c_uint32 * 8)(*end_ids[:8]))


class SplDfaIn(ctypes.Structure):
    """spl_dfa_in: the rows of ids, their lengths, the state words, the DFA table and its index, device addresses (None: not given)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("row_len", ctypes.c_uint32), ("n_seqs", ctypes.c_uint64), ("d_ids", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_state_in", ctypes.c_void_p), ("d_table", ctypes.c_void_p), ("d_index", ctypes.c_void_p),
                ("n_states", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def __init__(self, n_seqs=0, row_len=0, ids=None, lengths=None, state=None, table=None, index=None, n_states=0):
        super().__init__(ctypes.sizeof(SplDfaIn), row_len, n_seqs, ids, lengths, state, table, index, n_states, 0)


class SplDfaOut(ctypes.Structure):
    """spl_dfa_out: where the outputs go, device addresses (None: not wanted)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("d_state_out", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("d_live", ctypes.c_void_p)]

    def __init__(self, state=None, mask=None, live=None):
        super().__init__(ctypes.sizeof(SplDfaOut), 0, state, mask, live)


class SplDfaJumpOut(ctypes.Structure):
    """spl_dfa_jump_out: the jump index and where the emitted ids and their counts go, device addresses."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("row_len_out", ctypes.c_uint32), ("d_jump_index", ctypes.c_void_p), ("d_forced_ids", ctypes.c_void_p),
                ("d_forced_len", ctypes.c_void_p)]

    def __init__(self, row_len_out=0, jump_index=None, forced_ids=None, forced_len=None):
        super().__init__(ctypes.sizeof(SplDfaJumpOut), row_len_out, jump_index, forced_ids, forced_len)


class SplNestOpts(ctypes.Structure):
    """spl_nest_opts (include/splintr_hip.h): flags, the words of a mask row, the END ids by value and the deepest stack."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("n_end", ctypes.c_uint32),
                ("end_ids", ctypes.c_uint32 * 8), ("max_depth", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def __init__(self, flags=0, n_words=0, end_ids=(), max_depth=0):
        end_ids = tuple(end_ids)
        super().__init__(ctypes.sizeof(SplNestOpts), flags, n_words, len(end_ids), (ctypes.c_uint32 * 8)(*end_ids[:8]), max_depth, 0)


class SplNestIn(ctypes.Structure):
    """spl_nest_in: the rows of ids, their lengths, the state rows, the nest table and its index, device addresses (None: not given)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("row_len", ctypes.c_uint32), ("n_seqs", ctypes.c_uint64), ("d_ids", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_state_in", ctypes.c_void_p), ("d_table", ctypes.c_void_p), ("d_index", ctypes.c_void_p),
                ("n_states", ctypes.c_uint32), ("n_ret", ctypes.c_uint32), ("dep_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("index_bytes", ctypes.c_uint64)]

    def __init__(self, n_seqs=0, row_len=0, ids=None, lengths=None, state=None, table=None, index=None, n_states=0, n_ret=0, dep_cap=0, index_bytes=0):
        super().__init__(ctypes.sizeof(SplNestIn), row_len, n_seqs, ids, lengths, state, table, index, n_states, n_ret, dep_cap, 0, index_bytes)


class SplNestOut(ctypes.Structure):
    """spl_nest_out: where the outputs go, device addresses (None: not wanted)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("d_state_out", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("d_live", ctypes.c_void_p)]

    def __init__(self, state=None, mask=None, live=None):
        super().__init__(ctypes.sizeof(SplNestOut), 0, state, mask, live)


class SplDraftOut(ctypes.Structure):
    """spl_draft_out: the draft's parents (None: a chain) and where the rows of a draft call go, device addresses (None: not wanted)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("d_parent", ctypes.c_void_p), ("d_mask", ctypes.c_void_p),
                ("d_ok", ctypes.c_void_p), ("d_live", ctypes.c_void_p), ("d_state_out", ctypes.c_void_p)]

    def __init__(self, flags=0, parent=None, mask=None, ok=None, live=None, state=None):
        super().__init__(ctypes.sizeof(SplDraftOut), flags, parent, mask, ok, live, state)


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). splintr_amd has no CPU fallback.")
    # ONE HIP runtime per process: torch ships its own copy of libamdhip64 and loads it by path; if
    # this library pulled in /opt/rocm's copy first, torch's would come up second and find the GPU's
    # VM already acquired ("No HIP GPUs are available").  With torch imported first both resolve to
    # the copy that is already loaded (same SONAME).  torch is optional for the encode path itself.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), \
        ctypes.POINTER(ctypes.c_uint64)
    L.spl_last_error.restype = ctypes.c_char_p
    L.spl_device_count.restype = ctypes.c_int
    L.spl_create.restype = vp
    L.spl_create.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.POINTER(SplOpts)]
    L.spl_add_special.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32]
    L.spl_vocab_size.restype = ctypes.c_uint32
    L.spl_vocab_size.argtypes = [vp]
    L.spl_destroy.argtypes = [vp]
    L.spl_destroy.restype = None
    L.spl_reserve.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64]
    L.spl_set_devices.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32]
    L.spl_n_devices.restype = ctypes.c_uint32
    L.spl_n_devices.argtypes = [vp]
    L.spl_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    L.spl_host_alloc.restype = vp
    L.spl_host_alloc.argtypes = [ctypes.c_size_t]
    L.spl_host_free.restype = None
    L.spl_host_free.argtypes = [vp]
    L.spl_token_bytes.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32)]
    L.spl_is_byte_level.argtypes = [vp]
    L.spl_encode_batch.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.spl_result_tokens.restype = u32p
    L.spl_result_tokens.argtypes = [vp]
    L.spl_result_offsets.restype = u64p
    L.spl_result_offsets.argtypes = [vp]
    L.spl_result_n_tokens.restype = ctypes.c_uint64
    L.spl_result_n_tokens.argtypes = [vp]
    L.spl_result_n_docs.restype = ctypes.c_uint64
    L.spl_result_n_docs.argtypes = [vp]
    L.spl_result_free.argtypes = [vp]
    L.spl_result_free.restype = None
    L.spl_encode_batch_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint32, vp,
                                          ctypes.c_uint64, vp, vp]
    L.spl_decode_batch.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(u8p), ctypes.POINTER(u64p)]
    L.spl_free.argtypes = [vp]
    L.spl_free.restype = None
    L.spl_profile_enable.argtypes = [vp, ctypes.c_int]
    L.spl_profile_reset.argtypes = [vp]
    L.spl_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    L.spl_kernel_name.restype = ctypes.c_char_p
    L.spl_kernel_name.argtypes = [ctypes.c_int]
    L.spl_last_queue_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    L.spl_debug_phases.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    L.spl_debug_blocks.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.spl_debug_rebase_offsets.argtypes = [vp, vp, u64p, ctypes.c_uint32, vp]
    L.spl_gatherv_pack.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint64, vp]
    L.spl_gatherv_unpack.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, vp, ctypes.c_uint64, vp,
                                     vp, vp]
    L.spl_encode_batch_device_packed.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_uint32, vp,
                                                 ctypes.c_uint64, vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp]
    L.spl_gatherv_unpack_group.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                           ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp]
    L.spl_split_host.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, vp]
    L.spl_split_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.spl_device_split_fallbacks.restype = ctypes.c_uint64
    L.spl_device_split_fallbacks.argtypes = [vp]
    L.spl_small_path_calls.restype = ctypes.c_uint64
    L.spl_small_path_calls.argtypes = [vp]
    L.spl_pick_stream.restype = ctypes.c_int
    L.spl_pick_stream.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)]
    L.spl_encode_chunks_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64, vp, vp]
    L.spl_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.spl_comm_create.restype = vp
    L.spl_comm_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.spl_comm_destroy.restype = None
    L.spl_comm_destroy.argtypes = [vp]
    L.spl_comm_rank.argtypes = [vp]
    L.spl_comm_world.argtypes = [vp]
    L.spl_allgather_slabs.argtypes = [vp, vp, vp, ctypes.c_uint64, vp]
    L.spl_allgather_slabs_p2p.argtypes = [vp, vp, vp, ctypes.c_uint64, vp]
    L.spl_gatherv_unpack_at.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                        vp, vp, vp]
    L.spl_allgatherv_csr.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                     u64p, u64p, vp]
    L.spl_pad_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplCollateOpts), vp, vp, vp, vp]
    L.spl_pack_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplCollateOpts), vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.spl_pair_device.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplPairOpts),
                                  vp, vp, vp, vp, vp, vp, vp, vp]
    L.spl_chat_work_bytes.restype = ctypes.c_uint64
    L.spl_chat_work_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    L.spl_chat_device.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(SplChatOpts)] + \
        [vp] * 12
    L.spl_seqpack_work_bytes.restype = ctypes.c_uint64
    L.spl_seqpack_work_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    L.spl_seqpack_device.argtypes = [vp, ctypes.POINTER(SplSeqpackIn), ctypes.POINTER(SplSeqpackOpts), ctypes.POINTER(SplSeqpackOut), vp, vp]
    L.spl_window_work_bytes.restype = ctypes.c_uint64
    L.spl_window_work_bytes.argtypes = [ctypes.c_uint64]
    L.spl_window_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplCollateOpts), ctypes.c_uint32, vp, ctypes.c_uint64,
                                    vp, vp, vp, vp, vp, vp, vp, vp]
    L.spl_decode_reserve_device.argtypes = [vp, ctypes.c_uint64]
    L.spl_decode_batch_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplDecodeOpts), vp,
                                          ctypes.c_uint64, vp, vp]
    L.spl_max_token_bytes.restype = ctypes.c_uint32
    L.spl_max_token_bytes.argtypes = [vp]
    L.spl_token_spans_device.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplDecodeOpts), ctypes.c_uint32,
                                         vp, vp, vp, vp, vp]
    L.spl_stream_reserve_device.argtypes = [vp, ctypes.c_uint64]
    L.spl_stream_decode_device.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(SplDecodeOpts), ctypes.c_uint32, vp, vp, vp, vp,
                                           ctypes.c_uint64, vp, vp]
    L.spl_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    L.spl_stop_reserve_device.argtypes = [vp, ctypes.c_uint64]
    L.spl_stop_match_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64,
                                        vp, vp, vp]
    L.spl_heal_reserve_device.argtypes = [vp, ctypes.c_uint64]
    L.spl_heal_begin_device.argtypes = [vp, ctypes.POINTER(SplHealIn), ctypes.POINTER(SplHealOpts), ctypes.POINTER(SplHealOut), vp]
    L.spl_heal_step_device.argtypes = [vp, ctypes.POINTER(SplHealIn), ctypes.POINTER(SplHealOpts), ctypes.POINTER(SplHealOut), vp]
    L.spl_utf8_mask_reserve_device.argtypes = [vp]
    L.spl_utf8_mask_device.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(SplDecodeOpts), ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    L.spl_mask_apply_device.argtypes = [vp, ctypes.POINTER(SplMaskApply), vp]
    L.spl_choice_reserve_device.argtypes = [vp]
    L.spl_choice_step_device.argtypes = [vp, ctypes.POINTER(SplChoiceIn), ctypes.POINTER(SplChoiceOpts), ctypes.POINTER(SplChoiceOut), vp]
    L.spl_dfa_reserve_device.argtypes = [vp]
    L.spl_dfa_index_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.spl_dfa_step_device.argtypes = [vp, ctypes.POINTER(SplDfaIn), ctypes.POINTER(SplDfaOpts), ctypes.POINTER(SplDfaOut), vp]
    L.spl_dfa_jump_index_device.argtypes = [vp, vp, ctypes.c_uint32, vp, vp]
    L.spl_dfa_jump_device.argtypes = [vp, ctypes.POINTER(SplDfaIn), ctypes.POINTER(SplDfaOpts), ctypes.POINTER(SplDfaOut), ctypes.POINTER(SplDfaJumpOut), vp]
    L.spl_nest_reserve_device.argtypes = [vp]
    L.spl_nest_index_device.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), vp]
    L.spl_nest_step_device.argtypes = [vp, ctypes.POINTER(SplNestIn), ctypes.POINTER(SplNestOpts), ctypes.POINTER(SplNestOut), vp]
    L.spl_dfa_draft_device.argtypes = [vp, ctypes.POINTER(SplDfaIn), ctypes.POINTER(SplDfaOpts), ctypes.POINTER(SplDraftOut), vp]
    L.spl_nest_draft_device.argtypes = [vp, ctypes.POINTER(SplNestIn), ctypes.POINTER(SplNestOpts), ctypes.POINTER(SplDraftOut), vp]
    _lib = L
    return L


_shim = None


def shim():
    """The CPython front end (csrc/spl_pyshim.c): list[str] -> pinned UTF-8, list[list[int]] from the
    pinned CSR, one C call per encode.  Built by __graft_entry__.build(); no fallback."""
    global _shim
    if _shim is None:
        lib()                                   # libsplintr_hip.so first: the shim links against it
        from . import _spl_py
        _shim = _spl_py
    return _shim


def last_error() -> str:
    return (lib().spl_last_error() or b"").decode("utf-8", "replace")
