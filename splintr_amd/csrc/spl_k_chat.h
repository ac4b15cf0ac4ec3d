// spl_k_chat.h -- from a CSR of MESSAGES (ids[T] u32, off[n_docs + 1] u64) to one row per CONVERSATION, two launches:
//
//   k_chat_turns     a WAVEFRONT owns a conversation: the extents of its turns (header + content + footer by the turn's role) are scanned
//                    into start[t], the oldest turns are dropped until the rest fits (SPL_CHAT_DROP_OLDEST), and one record per
//                    conversation says what the gather needs: the first kept turn, the body offset subtracted, the kept length.  It
//                    also writes len, kept, turn_col and the status, and one workgroup copies the template out of the kernel argument.
//   k_collate_chat   rows[n_convs, L]: row c = bos + body' + gen, the rest pad_id; labels, loss mask, attention mask, role ids,
//                    special-token mask.  The gather of spl_k_pair.h's shape: a lane owns COL_VEC consecutive flat elements, a
//                    workgroup COL_SPAN of them, the grid is cpair_grid's and there is no loop over spans.
//
// No atomics, no polling, no workgroup waits for another; every output element is written once, by the lane that owns it.  The work
// buffer (chat_work_bytes) holds the template copy, the records and start[]: the second launch reads what the first wrote, in stream order.
//
// The mapping code is the plain C++ of the first half of this file (values and pointers only): tests/hostsim/chat_sim.cpp includes it
// in a g++ build, evaluates the gather for every output element and restates the wavefront walk of k_chat_turns lane by lane; the
// kernels below call exactly these functions.
//
// The template travels BY VALUE as an argument of k_chat_turns only.  A lane of the gather needs the entry of ITS column: indexing a
// by-value struct with a lane's own number makes the compiler copy the struct to scratch memory (spl_k_pair.h walks its 96 entries with a
// uniform index instead; 216 entries a group is too many for that).  So workgroup 0 of the first launch walks the template once with a
// uniform index -- scalar loads of the kernel argument, one vector store per lane -- and the gather indexes the copy in device memory.
// The per-role COUNTS never touch memory: eight header counts of 0..16 are 5 bits each in one 64-bit word, eight footer counts of 0..8
// are 4 bits each in a 32-bit word, and a lane shifts by its own role.
#pragma once
#include "spl_k_pair.h"
#include "spl_k_seqscan.h"

namespace spl {

// (the values of SPL_CHAT_* in include/splintr_hip.h; COL_I64 and COL_PAD_LEFT are shared with the collate family)
constexpr uint32_t CHAT_DROP_OLDEST = 32u, CHAT_PIN_FIRST = 64u;
constexpr uint32_t CHAT_MAX_ROLES = 8, CHAT_MAX_HEADER = 16, CHAT_MAX_FOOTER = 8, CHAT_MAX_BOS = 8, CHAT_MAX_GEN = 16;
constexpr uint32_t CHAT_NO_ROLE = 255;
constexpr uint32_t CHAT_WAVES = 4;                  // conversations per workgroup of k_chat_turns (one per wavefront)
// the template as one array of words: header[r][j] at r * 16 + j, footer[r][j] at 128 + r * 8 + j, bos at 192, gen at 200
constexpr uint32_t CHAT_TPL_WORDS = 256, CHAT_TPL_FOOTER = CHAT_MAX_ROLES * CHAT_MAX_HEADER, CHAT_TPL_BOS = CHAT_TPL_FOOTER + CHAT_MAX_ROLES * CHAT_MAX_FOOTER,
                   CHAT_TPL_GEN = CHAT_TPL_BOS + CHAT_MAX_BOS;
static_assert(CHAT_TPL_GEN + CHAT_MAX_GEN <= CHAT_TPL_WORDS && CHAT_TPL_WORDS == COL_NT, "one word per lane of the copying workgroup");

struct ChatTpl { uint32_t w[CHAT_TPL_WORDS]; };
struct ChatGeo {
    uint32_t flags, L, pad_id, ignore_id;
    uint32_t n_bos, n_gen, n_roles, train_content, train_footer;
    uint32_t ftr_pack;                                // n_footer[r] in bits 4r .. 4r + 3
    uint64_t hdr_pack;                                // n_header[r] in bits 5r .. 5r + 4
};
struct ChatSrc {
    const uint32_t* ids; const uint64_t* off;
    const int32_t* turn_doc; const uint8_t* turn_role; const uint8_t* turn_train; const uint64_t* conv_off;
    uint32_t n_docs, n_turns, n_convs;                // (all below 2^31: the C ABI refuses more)
};
// what k_chat_turns leaves the gather for one conversation (32 bytes)
struct ChatRec {
    uint64_t sub;             // body position q (q >= pin) is position q + sub of the WHOLE body, the one start[] counts in
    uint32_t t_first, n;      // the conversation's first turn and its number of turns (0: none, or a bad range)
    uint32_t t0;              // the first kept turn (relative; behind the pinned turn 0 when pinned)
    uint32_t kept;            // body entries in the row, at most the budget
    uint32_t pin;             // body positions below it are turn 0's own (pinned: min(its extent, the budget); otherwise 0)
    uint32_t pinned;          // 1: turn 0 is kept in front of the turns from t0 >= 1 on
};
static_assert(sizeof(ChatRec) == 32, "two 16-byte loads");
// one turn, resolved
struct ChatTurn {
    uint64_t o0, len;         // its content: ids[o0 .. o0 + len)
    uint32_t r, nh, nf;       // role, header and footer entries (a bad role: 0 and 0)
    bool bad, trained;        // a role or a document index out of range; content (and, by the role, footer) entries are labels
};

SPL_HD uint32_t chat_nh(const ChatGeo& g, uint32_t r) { return (uint32_t)(g.hdr_pack >> (5 * r)) & 31u; }
SPL_HD uint32_t chat_nf(const ChatGeo& g, uint32_t r) { return (g.ftr_pack >> (4 * r)) & 15u; }
SPL_HD uint32_t chat_budget(const ChatGeo& g) { return g.L - g.n_bos - g.n_gen; }
// (host) the counts of the C ABI's options into the two packed words
inline void chat_set_counts(ChatGeo& g, const uint32_t* n_header, const uint32_t* n_footer) {
    g.hdr_pack = 0; g.ftr_pack = 0;
    for (uint32_t r = 0; r < g.n_roles; r++) { g.hdr_pack |= (uint64_t)n_header[r] << (5 * r); g.ftr_pack |= n_footer[r] << (4 * r); }
}

// ------------------------------------------------------------------------------------------ the work buffer
SPL_HD uint64_t chat_work_bytes(uint64_t n_turns, uint64_t n_convs) {
    return (CHAT_TPL_WORDS * 4 + n_convs * sizeof(ChatRec) + n_turns * 8 + 15) / 16 * 16;
}
SPL_HD uint32_t* chat_work_tpl(void* work) { return static_cast<uint32_t*>(work); }
SPL_HD ChatRec* chat_work_rec(void* work) { return reinterpret_cast<ChatRec*>(static_cast<uint8_t*>(work) + CHAT_TPL_WORDS * 4); }
SPL_HD uint64_t* chat_work_start(void* work, uint32_t n_convs) { return reinterpret_cast<uint64_t*>(chat_work_rec(work) + n_convs); }

// ------------------------------------------------------------------------------------------ turns and conversations
// turn T (absolute).  A role >= n_roles: the turn contributes nothing; a document index outside 0 .. n_docs - 1: its content is empty.
SPL_HD ChatTurn chat_turn(const ChatSrc& s, const ChatGeo& g, uint32_t T) {
    ChatTurn u;
    u.o0 = 0; u.len = 0; u.nh = 0; u.nf = 0; u.bad = false; u.trained = false;
    u.r = s.turn_role[T];
    if (u.r >= g.n_roles) { u.bad = true; return u; }
    u.nh = chat_nh(g, u.r); u.nf = chat_nf(g, u.r);
    uint32_t d = T;                                               // (turn_doc == null: T < n_docs, the host has checked n_turns <= n_docs)
    if (s.turn_doc) d = (uint32_t)s.turn_doc[T];
    if (d >= s.n_docs) u.bad = true;                              // (a negative index is at least 2^31 as an unsigned number, n_docs is below that)
    else { u.o0 = s.off[d]; u.len = s.off[d + 1] - u.o0; }
    u.trained = ((g.train_content >> u.r) & 1u) != 0;
    if (s.turn_train) { if (s.turn_train[T] == 0) u.trained = false; }
    return u;
}
SPL_HD uint64_t chat_ext(const ChatTurn& u) { return u.nh + u.len + u.nf; }

// conversation c: its turns [t_first, t_first + n); a range that is reversed or reaches beyond n_turns has none and is reported
SPL_HD bool chat_conv(const ChatSrc& s, uint32_t c, uint32_t& t_first, uint32_t& n) {
    const uint64_t a = s.conv_off[c], b = s.conv_off[c + 1];
    const bool bad = b < a || b > s.n_turns;
    t_first = bad ? 0u : (uint32_t)a;
    n = bad ? 0u : (uint32_t)(b - a);
    return bad;
}

// DROP_OLDEST: "the body fits from turn t on" -- S the whole body's length, start_t turn t's start in it, pe0 the pinned turn's extent
// (0: none).  start is non-decreasing in t, so the predicate is monotone: false ... false true ... true.
SPL_HD bool chat_fits(uint64_t S, uint64_t start_t, uint64_t pe0, uint32_t B) { return pe0 + (S - start_t) <= B; }

// the record: t0 / start_t0 = the first kept turn and its start (0, 0 without DROP_OLDEST), e0 = turn 0's extent
SPL_HD ChatRec chat_rec(const ChatGeo& g, uint32_t t_first, uint32_t n, uint64_t S, uint32_t t0, uint64_t start_t0, uint64_t e0) {
    ChatRec r;
    const uint32_t B = chat_budget(g);
    const bool pinned = (g.flags & CHAT_PIN_FIRST) && (g.flags & CHAT_DROP_OLDEST) && n >= 2;
    r.t_first = t_first; r.n = n; r.t0 = t0; r.pinned = pinned ? 1u : 0u;
    r.pin = pinned ? (e0 < B ? (uint32_t)e0 : B) : 0u;
    r.sub = pinned ? start_t0 - e0 : start_t0;                    // (t0 >= 1 when pinned: start_t0 >= e0)
    const uint64_t rest = S - r.sub;
    r.kept = rest < B ? (uint32_t)rest : B;
    return r;
}
SPL_HD uint32_t chat_dropped(const ChatRec& r) { return r.t0 - r.pinned; }
SPL_HD uint32_t chat_used(const ChatGeo& g, const ChatRec& r) { return g.n_bos + r.kept + g.n_gen; }
SPL_HD uint32_t chat_lead(const ChatGeo& g, const ChatRec& r) { return (g.L - chat_used(g, r)) * ((g.flags / COL_PAD_LEFT) & 1u); }
SPL_HD int32_t chat_sat31(uint64_t x) { return x < 0x7FFFFFFFull ? (int32_t)x : 0x7FFFFFFF; }

// the columns [c0, c1) of turn t's CONTENT in its row, clipped to the row; (-1, -1): dropped, wholly behind the cut, or a bad turn
SPL_HD void chat_turn_cols(const ChatGeo& g, const ChatRec& r, uint32_t t, uint64_t start_t, const ChatTurn& u, int32_t& c0, int32_t& c1) {
    c0 = -1; c1 = -1;
    const bool first = r.pinned && t == 0;
    if (u.bad || (t < r.t0 && !first)) return;
    const uint64_t pb = first ? (uint64_t)u.nh : start_t + u.nh - r.sub;
    if (pb >= r.kept) return;
    const uint64_t pe = pb + u.len < r.kept ? pb + u.len : (uint64_t)r.kept;
    const uint32_t base = chat_lead(g, r) + g.n_bos;
    c0 = (int32_t)(base + (uint32_t)pb); c1 = (int32_t)(base + (uint32_t)pe);
}

// ------------------------------------------------------------------------------------------ one element of the gather
constexpr uint32_t CHAT_MASK = 1u, CHAT_LOSS = 2u, CHAT_SPECIAL = 4u;
// the turn of a row's previous body element: the next element's search starts there, and a turn is loaded once
struct ChatCur { uint32_t hint, t; bool have; uint64_t st; ChatTurn u; };

// the LARGEST t of [t_prev, n - 1] with start[t] <= p (start[t_prev] <= p holds): turns without entries share their start with their
// successor and are skipped.  Nearly always the next start lies beyond p and one read settles it.
SPL_HD uint32_t chat_locate(const uint64_t* start, uint32_t t_prev, uint32_t n, uint64_t p) {
    uint32_t lo = t_prev, hi = n - 1;
    if (lo == hi || start[lo + 1] > p) return lo;
    lo++;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (start[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// column c of the row of a conversation: the value, the role byte; returns CHAT_MASK | _LOSS | _SPECIAL.  start: the conversation's own
// (start_all + t_first); tpl: the template copy.
SPL_HD uint32_t chat_elem(const ChatSrc& s, const ChatGeo& g, const uint32_t* tpl, const ChatRec& r, const uint64_t* start, uint32_t c,
                          ChatCur& cur, uint32_t& val, uint32_t& role) {
    const uint32_t used = chat_used(g, r), lead = chat_lead(g, r);
    val = g.pad_id; role = CHAT_NO_ROLE;
    const uint32_t x = c - lead;
    if (c < lead || x >= used) return CHAT_SPECIAL;                                 // padding
    if (x < g.n_bos) { val = tpl[CHAT_TPL_BOS + x]; return CHAT_MASK | CHAT_SPECIAL; }
    const uint32_t q = x - g.n_bos;
    if (q >= r.kept) { val = tpl[CHAT_TPL_GEN + (q - r.kept)]; return CHAT_MASK | CHAT_SPECIAL; }
    uint32_t t = 0;
    uint64_t p = q;
    if (q >= r.pin) { p = q + r.sub; t = chat_locate(start, cur.hint, r.n, p); cur.hint = t; }
    if (!cur.have || t != cur.t) { cur.u = chat_turn(s, g, r.t_first + t); cur.st = start[t]; cur.t = t; cur.have = true; }
    const ChatTurn& u = cur.u;
    const uint64_t j = p - cur.st;
    // (never true for conversations with turn ranges of their own; ranges that OVERLAP -- one of them is then reversed, and reported --
    //  share entries of start[]: whatever such an entry holds, nothing is read beyond a turn's own extent)
    if (j >= chat_ext(u)) return CHAT_SPECIAL;
    role = u.r;
    if (j < u.nh) { val = tpl[u.r * CHAT_MAX_HEADER + (uint32_t)j]; return CHAT_MASK | CHAT_SPECIAL; }
    if (j < u.nh + u.len) { val = s.ids[u.o0 + (j - u.nh)]; return CHAT_MASK | (u.trained ? CHAT_LOSS : 0u); }
    val = tpl[CHAT_TPL_FOOTER + u.r * CHAT_MAX_FOOTER + (uint32_t)(j - u.nh - u.len)];
    return CHAT_MASK | CHAT_SPECIAL | ((u.trained && ((g.train_footer >> u.r) & 1u)) ? CHAT_LOSS : 0u);
}

// One lane's group: n (1..COL_VEC) flat elements from e0 on.  v[i]: the values; bits: byte i holds element i's CHAT_MASK | _LOSS |
// _SPECIAL; roles: byte i its role.  A group that crosses a row boundary reads the next conversation's record.
SPL_HD void chat_group(const ChatSrc& s, const ChatGeo& g, const uint32_t* tpl, const ChatRec* recs, const uint64_t* start_all, uint64_t e0,
                       uint32_t n, uint32_t v[COL_VEC], uint32_t& bits, uint32_t& roles) {
    uint64_t p; uint32_t c;
    col_rowcol(e0, g.L, p, c);
    bits = 0; roles = 0;
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) v[i] = g.pad_id;
    for (uint32_t first = 0; first < n; p++, c = 0) {
        const ChatRec r = recs[p];
        const uint64_t* start = start_all + r.t_first;
        const uint32_t room = g.L - c, cnt = n - first < room ? n - first : room;
        ChatCur cur{};                                  // (have = false: no turn loaded yet)
        cur.hint = r.t0;
#pragma unroll
        for (uint32_t i = 0; i < COL_VEC; i++) {
            if (i < first || i - first >= cnt) continue;
            uint32_t role;
            bits |= chat_elem(s, g, tpl, r, start, c + (i - first), cur, v[i], role) << (8 * i);
            roles |= role << (8 * i);
        }
        first += cnt;
    }
}

// a label: a trained entry holds its id (zero-extended in int64), every other entry ignore_id (SIGN-extended in int64: -100 is a number);
// int32 labels are the low word
SPL_HD int64_t chat_label(uint32_t v, bool trained, uint32_t ignore) { return trained ? (int64_t)(uint64_t)v : (int64_t)(int32_t)ignore; }

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------ launch 1: the turns
// grid: ceil(n_convs / CHAT_WAVES) workgroups of COL_NT lanes.  (tests/hostsim/chat_sim.cpp shares the functions above, NOT this walk:
// the three passes over a conversation's turns are restated there lane by lane.)
__global__ __launch_bounds__(COL_NT) void k_chat_turns(ChatSrc s, ChatGeo g, ChatTpl tpl, void* __restrict__ work, int32_t* __restrict__ len,
                                                       int32_t* __restrict__ kept, int32_t* __restrict__ turn_col, uint32_t* __restrict__ status) {
    if (blockIdx.x == 0) {                              // the template: a uniform index (scalar loads of the kernel argument), one store per lane
        uint32_t mine = 0;
        for (uint32_t j = 0; j < CHAT_TPL_WORDS; j++) {
            const uint32_t x = tpl.w[CPAIR_UNIFORM(j)];
            mine = threadIdx.x == j ? x : mine;
        }
        chat_work_tpl(work)[threadIdx.x] = mine;
    }
    const uint32_t lane = threadIdx.x & 63, c = blockIdx.x * CHAT_WAVES + (threadIdx.x >> 6);
    if (c >= s.n_convs) return;
    uint32_t t_first, n;
    if (chat_conv(s, c, t_first, n)) { if (lane == 0) status[0] = 1u; }
    uint64_t* start = chat_work_start(work, s.n_convs) + t_first;
    const uint32_t B = chat_budget(g);
    // 1. extents -> start[t], 64 turns at a time with a running carry; e0 = turn 0's extent, last = the last turn's start
    uint64_t S = 0, e0 = 0, last = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t t = base + lane;
        uint64_t ext = 0;
        if (t < n) {
            const ChatTurn u = chat_turn(s, g, t_first + t);
            ext = chat_ext(u);
            if (u.bad) status[0] = 1u;
        }
        const uint64_t x = wave_scan_incl64(ext), st = S + x - ext;
        if (t < n) start[t] = st;
        if (base == 0) e0 = (uint64_t)__shfl((unsigned long long)x, 0);
        const uint32_t l = n - 1 - base < 63 ? n - 1 - base : 63;
        last = (uint64_t)__shfl((unsigned long long)st, (int)l);
        S += (uint64_t)__shfl((unsigned long long)x, 63);
    }
    // 2. DROP_OLDEST: the smallest t from which the body fits -- a ballot and a find-first over each 64; none: the last turn
    uint32_t t0 = 0;
    uint64_t start_t0 = 0;
    if ((g.flags & CHAT_DROP_OLDEST) && n) {
        const bool pinned = (g.flags & CHAT_PIN_FIRST) && n >= 2;
        const uint64_t pe0 = pinned ? e0 : 0;
        bool found = false;
        for (uint32_t base = 0; base < n && !found; base += 64) {
            const uint32_t t = base + lane;
            const uint64_t st = t < n ? start[t] : 0;             // (this lane's own store of pass 1)
            const bool ok = t < n && t >= (pinned ? 1u : 0u) && chat_fits(S, st, pe0, B);
            const unsigned long long m = __ballot(ok);
            if (m) {
                const int l = __ffsll((long long)m) - 1;
                t0 = base + (uint32_t)l;
                start_t0 = (uint64_t)__shfl((unsigned long long)st, l);
                found = true;
            }
        }
        if (!found) { t0 = n - 1; start_t0 = last; }
    }
    const ChatRec r = chat_rec(g, t_first, n, S, t0, start_t0, e0);
    if (lane == 0) {
        chat_work_rec(work)[c] = r;
        if (len) len[c] = (int32_t)chat_used(g, r);
        if (kept) { kept[2 * (uint64_t)c] = (int32_t)chat_dropped(r); kept[2 * (uint64_t)c + 1] = chat_sat31(S - r.sub - r.kept); }
    }
    // 3. the columns of every turn's content
    if (turn_col) {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t t = base + lane;
            if (t >= n) break;
            const ChatTurn u = chat_turn(s, g, t_first + t);
            int32_t c0, c1;
            chat_turn_cols(g, r, t, start[t], u, c0, c1);
            *reinterpret_cast<int2*>(turn_col + 2 * (uint64_t)(t_first + t)) = make_int2(c0, c1);
        }
    }
}

// ------------------------------------------------------------------------------------------ launch 2: the gather
template <bool I64> __device__ __forceinline__ void chat_store_label(void* labels, uint64_t e, uint32_t v, bool trained, uint32_t ignore) {
    const int64_t y = chat_label(v, trained, ignore);
    if (I64) static_cast<int64_t*>(labels)[e] = y;
    else static_cast<uint32_t*>(labels)[e] = (uint32_t)y;
}
template <bool I64> __device__ __forceinline__ void chat_store_labels4(void* labels, uint64_t e, const uint32_t v[COL_VEC], uint32_t bits, uint32_t ignore) {
    uint32_t x[COL_VEC], hi[COL_VEC];
#pragma unroll
    for (uint32_t i = 0; i < COL_VEC; i++) {
        const uint64_t y = (uint64_t)chat_label(v[i], ((bits >> (8 * i)) & CHAT_LOSS) != 0, ignore);
        x[i] = (uint32_t)y; hi[i] = (uint32_t)(y >> 32);
    }
    if (I64) {
        uint4* q = reinterpret_cast<uint4*>(static_cast<uint64_t*>(labels) + e);
        q[0] = make_uint4(x[0], hi[0], x[1], hi[1]);
        q[1] = make_uint4(x[2], hi[2], x[3], hi[3]);
    } else {
        *reinterpret_cast<uint4*>(static_cast<uint32_t*>(labels) + e) = make_uint4(x[0], x[1], x[2], x[3]);
    }
}

// grid: cpair_grid(n_convs * L) -- one workgroup per span of COL_SPAN flat elements
template <bool I64>
__global__ __launch_bounds__(COL_NT) void k_collate_chat(ChatSrc s, ChatGeo g, void* __restrict__ work, void* __restrict__ rows,
                                                         void* __restrict__ labels, uint8_t* __restrict__ loss, uint8_t* __restrict__ mask,
                                                         uint8_t* __restrict__ role, uint8_t* __restrict__ special) {
    const uint64_t total = (uint64_t)s.n_convs * g.L;
    const uint64_t e0 = cpair_span(blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y) * COL_SPAN + (uint64_t)threadIdx.x * COL_VEC;
    if (e0 >= total) return;
    const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
    uint32_t v[COL_VEC], bits, roles;
    chat_group(s, g, chat_work_tpl(work), chat_work_rec(work), chat_work_start(work, s.n_convs), e0, n, v, bits, roles);
    // (The rows' tail is this kernel's own, NOT col_store_group: rows and labels share one test of n, and with the rows stored through
    //  the shared helper the kernel measured 1 .. 2 % slower than before -- profiles/shared_prims_ab.txt.  As written here it compiles
    //  to the code it had.  The byte arrays go through col_store_bytes.)
    if (n == COL_VEC) {
        col_store4<I64>(rows, e0, v);
        if (labels) chat_store_labels4<I64>(labels, e0, v, bits, g.ignore_id);
    } else {                                            // the final partial group: nothing is written past n_convs * L
        for (uint32_t i = 0; i < n; i++) {
            col_store1<I64>(rows, e0 + i, v[i]);
            if (labels) chat_store_label<I64>(labels, e0 + i, v[i], ((bits >> (8 * i)) & CHAT_LOSS) != 0, g.ignore_id);
        }
    }
    col_store_bytes(mask, e0, n, bits & 0x01010101u);           // (an output that is not wanted: one uniform test each)
    col_store_bytes(loss, e0, n, (bits >> 1) & 0x01010101u);
    col_store_bytes(special, e0, n, (bits >> 2) & 0x01010101u);
    col_store_bytes(role, e0, n, roles);
}
#endif  // __HIPCC__

}  // namespace spl
