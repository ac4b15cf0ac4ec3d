// words_sim.cpp -- TEST TOOL (not part of the product, never shipped in the package).
//
// The word classifiers of splintr_amd/csrc/spl_scan_words.h compiled with plain g++ and driven over generated words: what
// classify_word_text returns -- it tries the two-byte form classify_word_two first -- must be, bit for bit, what the general
// classify_word returns for the same three words; classify_word_two, called directly under classify_word_text's guard, must
// take every word whose bytes beyond ASCII are whole two-byte characters and decline every other one.  "Whole two-byte
// characters" is decided here by a byte loop of its own (takes()), not by the header's word arithmetic.
//   -DSPL_WORDS_SIM_BREAK=1 / =2 build the header's two deliberately wrong variants: the sweeps must report them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../splintr_amd/csrc/spl_scan_words.h"

using namespace spl;

namespace {

struct Sim {
    std::vector<uint16_t> s1;
    std::vector<uint8_t> s2;
    DeviceTables dt;
    KindEnt aent[3][128], kent[16];
};

enum { N_CASES, N_TEXT_DONE, N_TWO_TAKEN, N_MISMATCH, N_TWO_MISMATCH, N_DECLINED_WELL_FORMED, N_TOOK_MALFORMED, N_GUARD_VIOLATION, N_WELL_FORMED,
       N_MALFORMED, N_OVERLONG, N_OVERLONG_TAKEN, N_CHARS2, N_CHARS3, N_STATS };

uint32_t rd32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// 0: some byte beyond ASCII of the word b[4..8) is not part of a whole two-byte character; 1: all are; 2: all are, and a lead is 0xC0 / 0xC1.
// chars: the characters that touch the word.
int takes(const uint8_t* b, int& chars) {
    int r = 1;
    chars = 0;
    for (int k = 4; k < 8; k++) {
        const uint8_t c = b[k];
        if (c < 0x80) continue;
        if (c >= 0xC0 && c <= 0xDF) {
            if (b[k + 1] < 0x80 || b[k + 1] > 0xBF) return 0;
            if (c < 0xC2) r = 2;
            chars++;
        } else if (c <= 0xBF) {
            if (b[k - 1] < 0xC0 || b[k - 1] > 0xDF) return 0;
            if (b[k - 1] < 0xC2) r = 2;
            if (k == 4) chars++;
        } else {
            return 0;
        }
    }
    return r;
}

bool same(const WordKinds& a, const WordKinds& b) { return a.rec == b.rec && a.v0 == b.v0 && a.v1 == b.v1; }

void run_case(const Sim& s, int pat, const uint8_t* b, uint32_t ts16, int i0, int lo, int iT, uint64_t* st) {
    const uint32_t wp = rd32(b), tw = rd32(b + 4), wn = rd32(b + 8);
    const auto aent = [&](uint32_t c) { return s.aent[pat][c]; };
    const auto kent = [&](uint32_t c) { return s.kent[c]; };
    const auto ascii = [&](uint32_t c) { return cp_class(s.dt, c); };
    st[N_CASES]++;
    WordKinds a{0u, 0u, 0u};
    const bool done = classify_word_text(s.dt, pat, wp, tw, wn, ts16, aent, kent, i0, lo, iT, a);
    const WordKinds g = classify_word(s.dt, pat, wp, tw, wn, ts16, kent, ascii, (ts16 >> 4) & 0xFu, 0u, i0, 1 << 20, 1 << 20, lo, iT);
    st[N_TEXT_DONE] += done;
    if (done && !same(a, g)) st[N_MISMATCH]++;
    const bool guard = ((ts16 >> 1) & 0x3FFu) == 0u && i0 - 3 >= lo && i0 + 7 <= iT;
    if (!guard) {
        if (done) st[N_GUARD_VIOLATION]++;
        return;
    }
    int chars = 0;
    const int wf = takes(b, chars);
    WordKinds t{0u, 0u, 0u};
    const bool two = classify_word_two(s.dt, pat, wp, tw, wn, aent, kent, t);
    st[N_TWO_TAKEN] += two;
    if (two && !same(t, g)) st[N_TWO_MISMATCH]++;
    if (wf == 1) { st[N_WELL_FORMED]++; if (!two) st[N_DECLINED_WELL_FORMED]++; if (chars == 2) st[N_CHARS2]++; if (chars == 3) st[N_CHARS3]++; }
    if (wf == 2) { st[N_OVERLONG]++; st[N_OVERLONG_TAKEN] += two; }
    if (wf == 0) { st[N_MALFORMED]++; if (two) st[N_TOOK_MALFORMED]++; }
}

// the neighbours: ASCII letter, digit, space, newline, apostrophe, '/', a two-byte, a three-byte and a four-byte character, a stray
// continuation byte, a lead without its continuation
struct Nb { int n; uint8_t b[4]; };
const Nb NEIGHBOURS[] = {{1, {'a'}}, {1, {'7'}}, {1, {' '}}, {1, {'\n'}}, {1, {'\''}}, {1, {'/'}}, {2, {0xC3, 0xA9}}, {3, {0xE2, 0x80, 0x94}},
                         {4, {0xF0, 0x9F, 0x98, 0x80}}, {1, {0xA9}}, {1, {0xC3}}};
const int N_NEIGHBOURS = (int)(sizeof(NEIGHBOURS) / sizeof(NEIGHBOURS[0]));

const int I0 = 64;          // window index of the word in the sweeps that are away from every edge

}  // namespace

extern "C" {

void* ws_create(const uint8_t* ucls, int len) {
    if (len < 32 || memcmp(ucls, "SPLU", 4) != 0) return nullptr;
    Sim* s = new Sim();
    const uint32_t shift = rd32(ucls + 8), nblocks = rd32(ucls + 12);
    const size_t n1 = 0x110000u >> shift, n2 = (size_t)nblocks << shift;
    if ((size_t)len < 32 + n1 * 2 + n2) { delete s; return nullptr; }
    s->s1.resize(n1);
    memcpy(s->s1.data(), ucls + 32, n1 * 2);
    s->s2.assign(ucls + 32 + n1 * 2, ucls + 32 + n1 * 2 + n2);
    s->dt = DeviceTables{};
    s->dt.ucls_stage1 = s->s1.data(); s->dt.ucls_stage2 = s->s2.data(); s->dt.ucls_shift = shift; s->dt.cjk_fast = 0u;
    bool fast = true;
    for (uint32_t cp = 0x4E00; cp < 0xA000 && fast; cp++) fast = cp_class(s->dt, cp) == C_LO;
    for (uint32_t cp = 0xAC00; cp < 0xD7A4 && fast; cp++) fast = cp_class(s->dt, cp) == C_LO;
    s->dt.cjk_fast = fast ? 1u : 0u;
    for (int pat = 0; pat < 3; pat++)
        for (uint32_t c = 0; c < 128; c++) s->aent[pat][c] = ascii_entry(pat, c, cp_class(s->dt, c));
    for (uint32_t c = 0; c < 16; c++) s->kent[c] = kind_entry(c);
    return s;
}
void ws_destroy(void* p) { delete (Sim*)p; }
int ws_n_stats() { return N_STATS; }

// one word, for a test that wants to look at a single case: b[0..12) = wp, tw, wn.  out: rec, v0, v1 of classify_word_text (if it took
// the word), of classify_word, of classify_word_two (if it took the word); returns bit 0: classify_word_text took it, bit 1: classify_word_two did
int ws_one(void* p, int pat, const uint8_t* b, uint32_t ts16, int i0, int lo, int iT, uint32_t* out) {
    const Sim& s = *(Sim*)p;
    const uint32_t wp = rd32(b), tw = rd32(b + 4), wn = rd32(b + 8);
    const auto aent = [&](uint32_t c) { return s.aent[pat][c]; };
    const auto kent = [&](uint32_t c) { return s.kent[c]; };
    const auto ascii = [&](uint32_t c) { return cp_class(s.dt, c); };
    WordKinds a{0u, 0u, 0u}, t{0u, 0u, 0u};
    const bool done = classify_word_text(s.dt, pat, wp, tw, wn, ts16, aent, kent, i0, lo, iT, a);
    const WordKinds g = classify_word(s.dt, pat, wp, tw, wn, ts16, kent, ascii, (ts16 >> 4) & 0xFu, 0u, i0, 1 << 20, 1 << 20, lo, iT);
    const bool two = classify_word_two(s.dt, pat, wp, tw, wn, aent, kent, t);
    const uint32_t o[9] = {a.rec, a.v0, a.v1, g.rec, g.v0, g.v1, t.rec, t.v0, t.v1};
    memcpy(out, o, sizeof(o));
    return (done ? 1 : 0) | (two ? 2 : 0);
}

// Every lead 0xC0..0xDF with every continuation byte (U+0080..U+07FF and the overlong forms), the lead at b[3] .. b[7] (byte 3 of wp, bytes
// 0..3 of tw), every neighbour directly in front and directly behind; 'x' elsewhere.
void ws_sweep_positions(void* p, int pat, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    for (int lead = 0xC0; lead <= 0xDF; lead++)
        for (int cont = 0x80; cont <= 0xBF; cont++)
            for (int at = 3; at <= 7; at++)
                for (int f = 0; f < N_NEIGHBOURS; f++)
                    for (int h = 0; h < N_NEIGHBOURS; h++) {
                        uint8_t b[12];
                        memset(b, 'x', 12);
                        const Nb &nf = NEIGHBOURS[f], &nh = NEIGHBOURS[h];
                        for (int j = 0; j < nf.n; j++) if (at - nf.n + j >= 0) b[at - nf.n + j] = nf.b[j];
                        b[at] = (uint8_t)lead; b[at + 1] = (uint8_t)cont;
                        for (int j = 0; j < nh.n; j++) if (at + 2 + j < 12) b[at + 2 + j] = nh.b[j];
                        run_case(s, pat, b, 0u, I0, 0, 1 << 20, st);
                    }
}

// Several characters in one word: every tiling of b[3..9) by single ASCII bytes and two-byte characters of different classes -- [L C L C],
// [C L C L] + C, [a L C L] + C, [L C a L] + C, ... -- each in front of and behind ASCII and a continuation / lead byte at b[2] and b[9].
void ws_sweep_fillings(void* p, int pat, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    // e-acute (Ll), E-acute (Lu), superscript two (No), no-break space (Zs), combining acute (Mn), multiplication sign (Sm), Arabic-Indic
    // digit zero (Nd), Cyrillic zhe, Greek alpha, Hebrew alef, U+07FF, U+0080
    static const uint8_t CH[][2] = {{0xC3, 0xA9}, {0xC3, 0x89}, {0xC2, 0xB2}, {0xC2, 0xA0}, {0xCC, 0x81}, {0xC3, 0x97}, {0xD9, 0xA0},
                                    {0xD0, 0xB6}, {0xCE, 0xB1}, {0xD7, 0x90}, {0xDF, 0xBF}, {0xC2, 0x80}};
    static const uint8_t AS[] = {'a', ' ', '7', '\n'};
    const int NCH = (int)(sizeof(CH) / 2), NAS = (int)sizeof(AS);
    static const uint8_t EDGE[] = {'x', 0xA9, 0xC3};
    for (int tiling = 0; tiling < 64; tiling++) {           // bit j: a two-byte character starts at b[3 + j]
        int piece[6], np = 0, j = 0;
        bool ok = true;
        while (j < 6) {
            if ((tiling >> j) & 1) { if (j + 1 >= 6 || ((tiling >> (j + 1)) & 1)) { ok = false; break; } piece[np++] = 2; j += 2; }
            else { piece[np++] = 1; j += 1; }
        }
        if (!ok) continue;
        int radix[6], total = 1;
        for (int q = 0; q < np; q++) { radix[q] = piece[q] == 2 ? NCH : NAS; total *= radix[q]; }
        for (int code = 0; code < total; code++)
            for (int ef = 0; ef < 3; ef++)
                for (int eh = 0; eh < 3; eh++) {
                    uint8_t b[12];
                    memset(b, 'x', 12);
                    b[2] = EDGE[ef]; b[9] = EDGE[eh];
                    int c = code, at = 3;
                    for (int q = 0; q < np; q++) {
                        const int v = c % radix[q];
                        c /= radix[q];
                        if (piece[q] == 2) { b[at] = CH[v][0]; b[at + 1] = CH[v][1]; at += 2; }
                        else b[at++] = AS[v];
                    }
                    run_case(s, pat, b, 0u, I0, 0, 1 << 20, st);
                }
    }
}

// The guard: words the two-byte form takes (a character at each of the five positions, and [C L C L] + C), with every one of the 16
// text-start bits set alone, and with lo and iT at and next to the guard's edges (i0 - 3 >= lo, i0 + 7 <= iT).
void ws_sweep_guards(void* p, int pat, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    uint8_t base[6][12];
    for (int at = 3; at <= 7; at++) { memset(base[at - 3], 'x', 12); base[at - 3][at] = 0xC3; base[at - 3][at + 1] = 0xA9; }
    memset(base[5], 'x', 12);
    for (int at = 3; at <= 7; at += 2) { base[5][at] = 0xD0; base[5][at + 1] = 0xB6; }
    for (int q = 0; q < 6; q++) {
        for (int d = 0; d < 16; d++) run_case(s, pat, base[q], 1u << d, I0, 0, 1 << 20, st);
        for (int lo = I0 - 5; lo <= I0 - 1; lo++) run_case(s, pat, base[q], 0u, I0, lo, 1 << 20, st);
        for (int iT = I0 + 5; iT <= I0 + 9; iT++) run_case(s, pat, base[q], 0u, I0, 0, iT, st);
        run_case(s, pat, base[q], 0u, 3, 0, 1 << 20, st);          // the first word the guard lets through ...
        run_case(s, pat, base[q], 0u, 2, 0, 1 << 20, st);          // (no word starts here in the kernel: i0 is a multiple of 4; the guard's arithmetic all the same)
    }
}

}  // extern "C"
