// chat_sim.cpp -- TEST TOOL: the mapping functions of splintr_amd/csrc/spl_k_chat.h (the code k_chat_turns and k_collate_chat run)
// evaluated on the CPU.  The gather: for every output element, with the kernel's geometry -- the grid of cpair_grid, workgroups of
// COL_NT lanes, COL_VEC elements a lane, the final partial group stored element by element.  The turns: k_chat_turns' wavefront walk is
// RESTATED here lane by lane (64 lanes an iteration, the inclusive scan with its running carry, the ballot and find-first of
// DROP_OLDEST) over the same functions, the way seqscan_sim.h restates the sequence drivers; a change to the walk in the kernel is
// checked by tests/test_gpu_chat.py alone.  cs_groups evaluates single groups at any flat index (outputs no memory could hold).
// Built with g++; no GPU.
#include <cstdint>
#include <cstring>

#include "../../splintr_amd/csrc/spl_k_chat.h"

using namespace spl;

namespace {

struct Args {
    ChatSrc s; ChatGeo g; ChatTpl tpl;
};

Args make(const uint32_t* ids, const uint64_t* off, uint32_t n_docs, const int32_t* turn_doc, const uint8_t* turn_role, const uint8_t* turn_train,
          uint32_t n_turns, const uint64_t* conv_off, uint32_t n_convs, uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t ignore_id,
          uint32_t n_roles, uint32_t train_content, uint32_t train_footer, const uint32_t* n_header, const uint32_t* n_footer,
          const uint32_t* header /* [8][16] */, const uint32_t* footer /* [8][8] */, const uint32_t* bos, uint32_t n_bos, const uint32_t* gen,
          uint32_t n_gen) {
    Args a{};
    a.s = ChatSrc{ids, off, turn_doc, turn_role, turn_train, conv_off, n_docs, n_turns, n_convs};
    a.g.flags = flags; a.g.L = L; a.g.pad_id = pad_id; a.g.ignore_id = ignore_id; a.g.n_bos = n_bos; a.g.n_gen = n_gen; a.g.n_roles = n_roles;
    a.g.train_content = train_content; a.g.train_footer = train_footer;
    chat_set_counts(a.g, n_header, n_footer);
    for (uint32_t r = 0; r < n_roles; r++) {
        for (uint32_t j = 0; j < n_header[r]; j++) a.tpl.w[r * CHAT_MAX_HEADER + j] = header[r * CHAT_MAX_HEADER + j];
        for (uint32_t j = 0; j < n_footer[r]; j++) a.tpl.w[CHAT_TPL_FOOTER + r * CHAT_MAX_FOOTER + j] = footer[r * CHAT_MAX_FOOTER + j];
    }
    for (uint32_t j = 0; j < n_bos; j++) a.tpl.w[CHAT_TPL_BOS + j] = bos[j];
    for (uint32_t j = 0; j < n_gen; j++) a.tpl.w[CHAT_TPL_GEN + j] = gen[j];
    return a;
}

// k_chat_turns, restated: one "wavefront" of 64 lanes per conversation
void turns(const Args& a, void* work, int32_t* len, int32_t* kept, int32_t* turn_col, uint32_t* status) {
    const ChatSrc& s = a.s; const ChatGeo& g = a.g;
    memcpy(chat_work_tpl(work), a.tpl.w, sizeof a.tpl.w);                       // (workgroup 0's copy)
    const uint32_t B = chat_budget(g);
    for (uint32_t c = 0; c < s.n_convs; c++) {
        uint32_t t_first, n;
        if (chat_conv(s, c, t_first, n)) status[0] = 1u;
        uint64_t* start = chat_work_start(work, s.n_convs) + t_first;
        uint64_t S = 0, e0 = 0, last = 0;
        for (uint32_t base = 0; base < n; base += 64) {
            uint64_t ext[64], x[64], st[64];
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t t = base + lane;
                ext[lane] = 0;
                if (t < n) {
                    const ChatTurn u = chat_turn(s, g, t_first + t);
                    ext[lane] = chat_ext(u);
                    if (u.bad) status[0] = 1u;
                }
            }
            uint64_t run = 0;
            for (uint32_t lane = 0; lane < 64; lane++) { run += ext[lane]; x[lane] = run; }       // (wave_scan_incl64: inclusive)
            for (uint32_t lane = 0; lane < 64; lane++) {
                st[lane] = S + x[lane] - ext[lane];
                if (base + lane < n) start[base + lane] = st[lane];
            }
            if (base == 0) e0 = x[0];
            const uint32_t l = n - 1 - base < 63 ? n - 1 - base : 63;
            last = st[l];
            S += x[63];
        }
        uint32_t t0 = 0;
        uint64_t start_t0 = 0;
        if ((g.flags & CHAT_DROP_OLDEST) && n) {
            const bool pinned = (g.flags & CHAT_PIN_FIRST) && n >= 2;
            const uint64_t pe0 = pinned ? e0 : 0;
            bool found = false;
            for (uint32_t base = 0; base < n && !found; base += 64) {
                uint64_t m = 0, st[64];
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint32_t t = base + lane;
                    st[lane] = t < n ? start[t] : 0;
                    const bool ok = t < n && t >= (pinned ? 1u : 0u) && chat_fits(S, st[lane], pe0, B);
                    if (ok) m |= 1ull << lane;                                   // (__ballot)
                }
                if (m) {
                    const int l = __builtin_ffsll((long long)m) - 1;
                    t0 = base + (uint32_t)l; start_t0 = st[l]; found = true;
                }
            }
            if (!found) { t0 = n - 1; start_t0 = last; }
        }
        const ChatRec r = chat_rec(g, t_first, n, S, t0, start_t0, e0);
        chat_work_rec(work)[c] = r;
        if (len) len[c] = (int32_t)chat_used(g, r);
        if (kept) { kept[2 * (uint64_t)c] = (int32_t)chat_dropped(r); kept[2 * (uint64_t)c + 1] = chat_sat31(S - r.sub - r.kept); }
        if (turn_col) {
            for (uint32_t t = 0; t < n; t++) {
                const ChatTurn u = chat_turn(s, g, t_first + t);
                chat_turn_cols(g, r, t, start[t], u, turn_col[2 * (uint64_t)(t_first + t)], turn_col[2 * (uint64_t)(t_first + t) + 1]);
            }
        }
    }
}

}  // namespace

#define CS_SRC                                                                                                                              \
    const uint32_t *ids, const uint64_t *off, uint32_t n_docs, const int32_t *turn_doc, const uint8_t *turn_role, const uint8_t *turn_train,  \
        uint32_t n_turns, const uint64_t *conv_off, uint32_t n_convs, uint32_t flags, uint32_t L, uint32_t pad_id, uint32_t ignore_id,        \
        uint32_t n_roles, uint32_t train_content, uint32_t train_footer, const uint32_t *n_header, const uint32_t *n_footer,                  \
        const uint32_t *header, const uint32_t *footer, const uint32_t *bos, uint32_t n_bos, const uint32_t *gen, uint32_t n_gen
#define CS_PASS                                                                                                                             \
    ids, off, n_docs, turn_doc, turn_role, turn_train, n_turns, conv_off, n_convs, flags, L, pad_id, ignore_id, n_roles, train_content,       \
        train_footer, n_header, n_footer, header, footer, bos, n_bos, gen, n_gen

extern "C" {

void cs_geometry(uint32_t out[5]) { out[0] = COL_NT; out[1] = COL_VEC; out[2] = COL_SPAN; out[3] = CHAT_WAVES; out[4] = (uint32_t)sizeof(ChatRec); }
uint64_t cs_work_bytes(uint64_t n_turns, uint64_t n_convs) { return chat_work_bytes(n_turns, n_convs); }

// rows u32 [n_convs * L], labels i64 [n_convs * L]; loss / mask / role / special u8; len i32 [n_convs], kept i32 [2 * n_convs], turn_col
// i32 [2 * n_turns] (each but rows may be null); status: one word; work: cs_work_bytes(n_turns, n_convs) bytes
int cs_chat(CS_SRC, uint32_t* rows, int64_t* labels, uint8_t* loss, uint8_t* mask, uint8_t* role, uint8_t* special, int32_t* len, int32_t* kept,
            int32_t* turn_col, uint32_t* status, void* work) {
    const Args a = make(CS_PASS);
    turns(a, work, len, kept, turn_col, status);
    const uint64_t total = (uint64_t)n_convs * L;
    uint32_t gx, gy, gz;
    cpair_grid(total, gx, gy, gz);
    for (uint32_t bz = 0; bz < gz; bz++)
        for (uint32_t by = 0; by < gy; by++)
            for (uint32_t bx = 0; bx < gx; bx++)
                for (uint32_t lane = 0; lane < COL_NT; lane++) {
                    const uint64_t e0 = cpair_span(bx, by, bz, gx, gy) * COL_SPAN + (uint64_t)lane * COL_VEC;
                    if (e0 >= total) continue;
                    const uint32_t n = total - e0 < COL_VEC ? (uint32_t)(total - e0) : COL_VEC;
                    uint32_t v[COL_VEC], bits, roles;
                    chat_group(a.s, a.g, chat_work_tpl(work), chat_work_rec(work), chat_work_start(work, n_convs), e0, n, v, bits, roles);
                    for (uint32_t i = 0; i < n; i++) {
                        const uint32_t b = bits >> (8 * i);
                        rows[e0 + i] = v[i];
                        if (labels) labels[e0 + i] = chat_label(v[i], (b & CHAT_LOSS) != 0, ignore_id);
                        if (mask) mask[e0 + i] = (uint8_t)(b & 1u);
                        if (loss) loss[e0 + i] = (uint8_t)((b >> 1) & 1u);
                        if (special) special[e0 + i] = (uint8_t)((b >> 2) & 1u);
                        if (role) role[e0 + i] = (uint8_t)(roles >> (8 * i));
                    }
                }
    return 0;
}

// The turns, then the groups that start at the flat elements e0[0 .. count): v [count * COL_VEC], bits / roles [count] (a group's four
// bytes each).  Nothing of size n_convs * L exists.
int cs_groups(CS_SRC, const uint64_t* e0, uint32_t count, uint32_t* v, uint32_t* bits, uint32_t* roles, int32_t* len, int32_t* kept,
              int32_t* turn_col, uint32_t* status, void* work) {
    const Args a = make(CS_PASS);
    turns(a, work, len, kept, turn_col, status);
    const uint64_t total = (uint64_t)n_convs * L;
    for (uint32_t k = 0; k < count; k++) {
        if (e0[k] >= total || e0[k] % COL_VEC) return -1;
        const uint32_t n = total - e0[k] < COL_VEC ? (uint32_t)(total - e0[k]) : COL_VEC;
        chat_group(a.s, a.g, chat_work_tpl(work), chat_work_rec(work), chat_work_start(work, n_convs), e0[k], n, v + (uint64_t)k * COL_VEC, bits[k],
                   roles[k]);
    }
    return 0;
}

}  // extern "C"
