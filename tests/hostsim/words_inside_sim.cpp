// words_inside_sim.cpp -- TEST TOOL (not part of the product, never shipped in the package).
//
// The form of splintr_amd/csrc/spl_scan_words.h for the word that holds one whole two-byte character (word_inside +
// classify_word_inside over classify_word_ascii, as the classify loop of k_pretok calls them) compiled with plain g++ and
// compared, word by word and bit for bit, with the general classify_word.  Whether the form MAY take a word is decided here
// by a byte loop of its own (expect_take), not by the header's word arithmetic: where the form declines, that it had to;
// where it takes, that it was allowed to.  What the form never looks at -- the neighbouring words, the text-start bits
// around the word, the end of the staged text -- is varied under it.
//   -DSPL_WORDS_SIM_BREAK=3 / =4 build the header's two deliberately wrong variants of the form: the sweeps must report them.
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

enum { N_CASES, N_TAKEN, N_MISMATCH, N_DECLINED_WRONG, N_TOOK_WRONG, N_DECLINED_TS, N_DECLINED_EDGE, N_DECLINED_SHAPE, N_STATS };

uint32_t rd32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// Where a word sits: window index i0, corpus position of window index 0 (w0 < 0: the window begins before the corpus),
// first window index past the text iB, window size Wv, end of the staged text iT.
struct Place { int i0, w0, iB, Wv, iT; };

// The form's contract, byte by byte: 0 take; 1 the shape is not "one lead 110xxxxx in byte 0..2, its continuation behind
// it, two ASCII bytes"; 2 an edge (the ASCII branch's own conditions); 3 a text start on the continuation byte.
int expect_take(const uint8_t* w, uint32_t ts4, uint32_t sk4, const Place& pl) {
    int lead = -1, beyond = 0;
    for (int k = 0; k < 4; k++) {
        if (w[k] < 0x80) continue;
        beyond++;
        if (w[k] >= 0xC0 && w[k] <= 0xDF && lead < 0) lead = k;
    }
    if (beyond != 2 || lead < 0 || lead > 2 || w[lead + 1] < 0x80 || w[lead + 1] > 0xBF) return 1;
    if (sk4 != 0u || !(pl.i0 + 3 < pl.iB) || pl.w0 + pl.i0 < 0) return 2;
    if ((ts4 >> (lead + 1)) & 1u) return 3;
    return 0;
}

// One word as the classify loop sees it: b[0..12) = the word before, the word, the word behind; ts16 bit d = "a text starts at
// window index i0 - 4 + d" (bits 4..7 are the word's own ts4).
void run_case(const Sim& s, int pat, const uint8_t* b, uint32_t ts16, uint32_t sk4, const Place& pl, uint64_t* st) {
    const uint32_t wp = pl.i0 > 0 ? rd32(b) : 0u, tw = rd32(b + 4), wn = rd32(b + 8);
    const uint32_t ts4 = (ts16 >> 4) & 0xFu;
    const auto kent = [&](uint32_t c) { return s.kent[c]; };
    const auto ascii = [&](uint32_t c) { return cp_class(s.dt, c); };
    st[N_CASES]++;
    // the classify loop's ASCII branch (spl_k_pretok.h)
    const bool mid = sk4 == 0u && pl.i0 + 3 < pl.iB && pl.w0 + pl.i0 >= 0;
    uint32_t k = 0u;
    const bool ins = mid && (tw & 0x80808080u) && word_inside(tw, ts4, k);
    const int want = expect_take(b + 4, ts4, sk4, pl);
    if (!ins) {
        if (want == 0) st[N_DECLINED_WRONG]++;
        st[want == 3 ? N_DECLINED_TS : want == 2 ? N_DECLINED_EDGE : N_DECLINED_SHAPE] += want != 0;
        return;
    }
    st[N_TAKEN]++;
    if (want != 0) st[N_TOOK_WRONG]++;
    const KindEnt e[4] = {s.aent[pat][tw & 0x7Fu], s.aent[pat][(tw >> 8) & 0x7Fu], s.aent[pat][(tw >> 16) & 0x7Fu], s.aent[pat][(tw >> 24) & 0x7Fu]};
    const WordKinds a = classify_word_inside(s.dt, pat, tw, k, classify_word_ascii(e, ts4), kent);
    const int lo = pl.w0 < 0 ? -pl.w0 : 0;
    const WordKinds g = classify_word(s.dt, pat, wp, tw, wn, ts16, kent, ascii, ts4, sk4, pl.i0, pl.iB, pl.Wv, lo, pl.iT);
    if (a.rec != g.rec || a.v0 != g.v0 || a.v1 != g.v1) st[N_MISMATCH]++;
}

// One representative per class of ASCII byte, and the bytes the split patterns name: apostrophe, space, newline, carriage return, tab,
// a digit, a lower-case and an upper-case letter, punctuation, '/' (mistral's [\r\n/]*)
const uint8_t ASCII_SET[] = {'\'', ' ', '\n', '\r', '\t', '7', 'a', 'A', '.', '/'};
const int N_ASCII = (int)sizeof(ASCII_SET);

const int WV = 1024, WPAD = 32;
// The word at window index 0 (with the corpus beginning at it, and two bytes behind it: declined), at index 4 (with the corpus beginning
// at it, at index 0, and at index 6: declined), in the middle, the last full word of a text that ends inside the window at iB = 40
// (with iB = 39 the same word holds iB in its byte 3: declined), the word that holds iB in its byte 0, 1, 2 and 3, and the window's last word.
const Place PLACES[] = {{0, 0, WV, WV, WV + WPAD},   {0, -2, WV, WV, WV + WPAD}, {4, -4, WV, WV, WV + WPAD}, {4, 0, WV, WV, WV + WPAD},
                        {4, -6, WV, WV, WV + WPAD},  {64, 0, WV, WV, WV + WPAD}, {36, 0, 40, WV, 40},        {36, 0, 39, WV, 39},
                        {40, 0, 40, WV, 40},         {40, 0, 41, WV, 41},        {40, 0, 42, WV, 42},        {40, 0, 43, WV, 43},
                        {WV - 4, 0, WV, WV, WV + WPAD}};
const int N_PLACES = (int)(sizeof(PLACES) / sizeof(PLACES[0]));

// what stands around the word (never looked at by the form): ASCII, stray continuation bytes, leads of two- and three-byte characters
const uint8_t AROUND[] = {'x', 0xA9, 0xC3, 0xE2};
const int N_AROUND = (int)sizeof(AROUND);

}  // namespace

extern "C" {

void* wi_create(const uint8_t* ucls, int len) {
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
    for (int pat = 0; pat < 3; pat++)
        for (uint32_t c = 0; c < 128; c++) s->aent[pat][c] = ascii_entry(pat, c, cp_class(s->dt, c));
    for (uint32_t c = 0; c < 16; c++) s->kent[c] = kind_entry(c);
    return s;
}
void wi_destroy(void* p) { delete (Sim*)p; }
int wi_n_stats() { return N_STATS; }
int wi_n_places() { return N_PLACES; }
int wi_n_ascii() { return N_ASCII; }

// Every lead 0xC0..0xDF with every continuation byte, the lead at byte 0, 1 and 2 of the word, every pair of ASCII bytes of ASCII_SET in
// the other two bytes, each of the 16 values of ts4, at one place.  What lies around the word changes from case to case: the bytes
// before and behind it, and the text-start bits outside it (none, all).
void wi_sweep_pairs(void* p, int pat, int place, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    const Place& pl = PLACES[place];
    uint32_t n = 0;
    for (int lead = 0xC0; lead <= 0xDF; lead++)
        for (int cont = 0x80; cont <= 0xBF; cont++)
            for (int at = 0; at < 3; at++)
                for (int x = 0; x < N_ASCII; x++)
                    for (int y = 0; y < N_ASCII; y++)
                        for (uint32_t ts4 = 0; ts4 < 16; ts4++, n++) {
                            uint8_t b[12];
                            memset(b, AROUND[n % N_AROUND], 4);
                            memset(b + 8, AROUND[(n / N_AROUND) % N_AROUND], 4);
                            uint8_t* w = b + 4;
                            const uint8_t two[2] = {ASCII_SET[x], ASCII_SET[y]};
                            for (int k = 0, j = 0; k < 4; k++) w[k] = k == at ? (uint8_t)lead : k == at + 1 ? (uint8_t)cont : two[j++];
                            const uint32_t out = ((n / 16) & 1u) ? 0xFF0Fu : 0u;
                            run_case(s, pat, b, (ts4 << 4) | out, 0u, pl, st);
                        }
}

// Words the form must decline by their shape, and the ones it takes among them: every word over a small alphabet of ASCII, leads of two-,
// three- and four-byte characters and continuation bytes, each ts4, each special-literal span sk4 of one byte and none, at one place.
void wi_sweep_shapes(void* p, int pat, int place, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    const Place& pl = PLACES[place];
    static const uint8_t AL[] = {'a', ' ', 0xC3, 0xD0, 0xA9, 0x80, 0xE2, 0xF0, 0xC0};
    const int NA = (int)sizeof(AL);
    for (int code = 0; code < NA * NA * NA * NA; code++)
        for (uint32_t ts4 = 0; ts4 < 16; ts4++)
            for (uint32_t sk = 0; sk < 5; sk++) {
                uint8_t b[12];
                memset(b, 'x', 12);
                for (int k = 0, c = code; k < 4; k++, c /= NA) b[4 + k] = AL[c % NA];
                const uint32_t sk4 = sk ? 1u << (sk - 1u) : 0u;
                run_case(s, pat, b, (ts4 & ~sk4) << 4, sk4, pl, st);
            }
}

}  // extern "C"
