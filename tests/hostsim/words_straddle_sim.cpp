// words_straddle_sim.cpp -- TEST TOOL (not part of the product, never shipped in the package).
//
// The form of splintr_amd/csrc/spl_scan_words.h for the two words that one two-byte character straddles (straddle_shape +
// word_straddle + classify_word_straddle over classify_word_ascii, as the classify loop of k_pretok calls them) compiled with
// plain g++ and compared, word by word and bit for bit, with the general classify_word -- on BOTH words of the pair, the one
// with the lead in byte 3 and the one with the continuation in byte 0.  Whether the form MAY take a word is decided here by a
// byte loop of its own (expect_take), not by the header's word arithmetic: where the form declines, that it had to; where it
// takes, that it was allowed to.  What the form never looks at -- the far neighbouring word, the text-start bits around the
// pair, the end of the staged text -- is varied under it.
//   -DSPL_WORDS_SIM_BREAK=5 / =6 build the header's two deliberately wrong variants of the form: the sweeps must report them.
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

enum { N_CASES, N_TAKEN_LEAD, N_TAKEN_CONT, N_INSIDE, N_MISMATCH, N_DECLINED_WRONG, N_TOOK_WRONG, N_DECLINED_TS, N_DECLINED_EDGE, N_DECLINED_SHAPE, N_STATS };

uint32_t rd32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// Where the PAIR sits: window index i0 of the lead word (-4: the continuation word is the window's first, there is no word in front),
// corpus position of window index 0 (w0 < 0: the window begins before the corpus), first window index past the text iB, window size
// Wv, end of the staged text iT.
struct Place { int i0, w0, iB, Wv, iT; };

// The form's contract for the word at window index i0, byte by byte.  w: the word; prev: the byte in front of it (for the window's
// first word: of no window, an edge); next: the byte behind it; tsn / skn, skp: text-start and special-literal bits of those two bytes.  0 take; 1 the shape is neither
// "three ASCII bytes and a lead 110xxxxx in byte 3 with a continuation byte behind the word" nor "a continuation byte in byte 0 with a
// lead 110xxxxx in front of the word and three ASCII bytes"; 2 an edge or a span (the ASCII branch's own conditions, and the
// neighbouring byte's); 3 a text start on the continuation byte.  side: 1 lead word, 2 continuation word.
int expect_take(const uint8_t* w, int prev, int next, uint32_t ts4, uint32_t sk4, uint32_t tsn, uint32_t skn, uint32_t skp, int i0, const Place& pl,
                int& side) {
    int beyond = 0, at = -1;
    for (int k = 0; k < 4; k++)
        if (w[k] >= 0x80) { beyond++; at = k; }
    side = 0;
    if (beyond != 1) return 1;
    if (at == 3 && w[3] >= 0xC0 && w[3] <= 0xDF && next >= 0x80 && next <= 0xBF) side = 1;
    else if (at == 0 && w[0] <= 0xBF && prev >= 0xC0 && prev <= 0xDF) side = 2;
    else return 1;
    const int lo = pl.w0 < 0 ? -pl.w0 : 0;
    if (sk4 != 0u || !(i0 + 3 < pl.iB) || pl.w0 + i0 < 0) return 2;
    if (side == 1 && (skn || !(i0 + 4 < pl.iB))) return 2;
    if (side == 2 && (skp || i0 == 0 || i0 - 1 < lo)) return 2;
    if (side == 1 ? tsn != 0u : (ts4 & 1u) != 0u) return 3;
    return 0;
}

// One word as the classify loop sees it: wp, tw, wn = the word before, the word, the word behind; ts16 bit d = "a text starts at window
// index i0 - 4 + d" (bits 4..7 are the word's own ts4); sk12 likewise the special-literal bits of the three words.
void run_word(const Sim& s, int pat, const uint8_t* b, uint32_t ts16, uint32_t sk12, int i0, const Place& pl, uint64_t* st) {
    const uint32_t wp = i0 > 0 ? rd32(b) : 0u, tw = rd32(b + 4), wn = rd32(b + 8);
    const uint32_t ts4 = (ts16 >> 4) & 0xFu, sk4 = (sk12 >> 4) & 0xFu;
    const auto kent = [&](uint32_t c) { return s.kent[c]; };
    const auto ascii = [&](uint32_t c) { return cp_class(s.dt, c); };
    const int lo = pl.w0 < 0 ? -pl.w0 : 0;
    st[N_CASES]++;
    // the classify loop's ASCII branch (spl_k_pretok.h)
    const bool mid = sk4 == 0u && i0 + 3 < pl.iB && pl.w0 + i0 >= 0;
    const bool beyond = (tw & 0x80808080u) != 0u;
    uint32_t kin = 0u;
    const bool ins = mid && beyond && word_inside(tw, ts4, kin);
    uint32_t side = (mid && beyond && !ins) ? straddle_shape(tw) : 0u, nb = 0u;
    if (side) {
        // (the kernel reads the word and the two bits of window index q = i0 + 4, i0 - 1, or 0 for the window's first word)
        const int d = side == 1u ? 8 : i0 > 0 ? 3 : 4;
        nb = side == 1u ? wn : i0 > 0 ? wp : tw;
        side = word_straddle(side, nb, ts4, (ts16 >> d) & 1u, (sk12 >> d) & 1u, i0, pl.iB, lo);
    }
    int want_side = 0;
    const int want = expect_take(b + 4, b[3], b[8], ts4, sk4, (ts16 >> 8) & 1u, (sk12 >> 8) & 1u, (sk12 >> 3) & 1u, i0, pl, want_side);
    if (ins) { st[N_INSIDE]++; if (want == 0) st[N_DECLINED_WRONG]++; return; }
    if (!side) {
        if (want == 0) st[N_DECLINED_WRONG]++;
        st[want == 3 ? N_DECLINED_TS : want == 2 ? N_DECLINED_EDGE : N_DECLINED_SHAPE] += want != 0;
        return;
    }
    st[side == 1u ? N_TAKEN_LEAD : N_TAKEN_CONT]++;
    if (want != 0 || (uint32_t)want_side != side) st[N_TOOK_WRONG]++;
    const KindEnt e[4] = {s.aent[pat][tw & 0x7Fu], s.aent[pat][(tw >> 8) & 0x7Fu], s.aent[pat][(tw >> 16) & 0x7Fu], s.aent[pat][(tw >> 24) & 0x7Fu]};
    const WordKinds a = classify_word_straddle(s.dt, pat, tw, nb, side, classify_word_ascii(e, ts4), kent);
    const WordKinds g = classify_word(s.dt, pat, wp, tw, wn, ts16, kent, ascii, ts4, sk4, i0, pl.iB, pl.Wv, lo, pl.iT);
    if (a.rec != g.rec || a.v0 != g.v0 || a.v1 != g.v1) st[N_MISMATCH]++;
}

// The pair: b[0..16) = the word before the lead word, the lead word, the continuation word, the word behind it; ts20 bit d = "a text
// starts at window index i0 - 4 + d", sk20 the special-literal bits likewise.  Both words go through the loop's branch -- those the
// kernel classifies: window indices 0 .. Wv - 4.
void run_pair(const Sim& s, int pat, const uint8_t* b, uint32_t ts20, uint32_t sk20, const Place& pl, uint64_t* st) {
    if (pl.i0 <= 0) { ts20 &= ~0xFu; sk20 &= ~0xFu; }                     // (no bits before window index 0)
    if (pl.i0 < 0) { ts20 &= ~0xFFu; sk20 &= ~0xFFu; }
    if (pl.i0 >= 0) run_word(s, pat, b, ts20 & 0xFFFFu, sk20 & 0xFFFu, pl.i0, pl, st);
    if (pl.i0 + 4 < pl.Wv) run_word(s, pat, b + 4, ts20 >> 4, (sk20 >> 4) & 0xFFFu, pl.i0 + 4, pl, st);
}

// One representative per class of ASCII byte, and the bytes the split patterns name: apostrophe, space, newline, carriage return, tab,
// a digit, a lower-case and an upper-case letter, punctuation, '/' (mistral's [\r\n/]*)
const uint8_t ASCII_SET[] = {'\'', ' ', '\n', '\r', '\t', '7', 'a', 'A', '.', '/'};
const int N_ASCII = (int)sizeof(ASCII_SET);

const int WV = 1024, WPAD = 32;
// The pair's lead word at window index 0 with the corpus beginning at it; with the corpus beginning two, three and four bytes behind
// index 0 (the lead word is before the corpus: declined; the continuation word at index 4 has its lead at index 3: taken only where
// that byte exists); the continuation word as the window's FIRST word (no word in front: declined); in the middle; the lead word as the
// window's last (its continuation is not text of this window: declined); the lead word as the last full word of a text that ends at
// iB = 40 (declined), 41 (the corpus ends right behind the continuation byte: the lead word taken, the other not a full word) and 44
// (both taken).
const Place PLACES[] = {{0, 0, WV, WV, WV + WPAD},  {0, -2, WV, WV, WV + WPAD}, {0, -3, WV, WV, WV + WPAD}, {0, -4, WV, WV, WV + WPAD},
                        {-4, 0, WV, WV, WV + WPAD}, {64, 0, WV, WV, WV + WPAD}, {WV - 4, 0, WV, WV, WV + WPAD},
                        {36, 0, 40, WV, 40},        {36, 0, 41, WV, 41},        {36, 0, 44, WV, 44}};
const int N_PLACES = (int)(sizeof(PLACES) / sizeof(PLACES[0]));

// what stands in the far words (never looked at by the form): ASCII, stray continuation bytes, leads of two- and three-byte characters
const uint8_t AROUND[] = {'x', 0xA9, 0xC3, 0xE2};
const int N_AROUND = (int)sizeof(AROUND);

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
    for (int pat = 0; pat < 3; pat++)
        for (uint32_t c = 0; c < 128; c++) s->aent[pat][c] = ascii_entry(pat, c, cp_class(s->dt, c));
    for (uint32_t c = 0; c < 16; c++) s->kent[c] = kind_entry(c);
    return s;
}
void ws_destroy(void* p) { delete (Sim*)p; }
int ws_n_stats() { return N_STATS; }
int ws_n_places() { return N_PLACES; }
int ws_n_ascii() { return N_ASCII; }

// Every lead 0xC0..0xDF with every continuation byte, every pair of ASCII bytes of ASCII_SET directly before the lead and directly behind
// the continuation, the text-start bits ON the lead and ON the continuation byte (window index i0 + 4) in their four combinations, at one
// place.  The other ASCII bytes of the two words, the far words and the text-start bits outside the pair change from case to case.
void ws_sweep_pairs(void* p, int pat, int place, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    const Place& pl = PLACES[place];
    uint32_t n = 0;
    for (int lead = 0xC0; lead <= 0xDF; lead++)
        for (int cont = 0x80; cont <= 0xBF; cont++)
            for (int x = 0; x < N_ASCII; x++)
                for (int y = 0; y < N_ASCII; y++)
                    for (uint32_t t = 0; t < 4; t++, n++) {
                        uint8_t b[16];
                        memset(b, AROUND[n % N_AROUND], 4);
                        memset(b + 12, AROUND[(n / N_AROUND) % N_AROUND], 4);
                        b[4] = ASCII_SET[n % N_ASCII]; b[5] = ASCII_SET[(n / 3) % N_ASCII]; b[6] = ASCII_SET[x]; b[7] = (uint8_t)lead;
                        b[8] = (uint8_t)cont; b[9] = ASCII_SET[y]; b[10] = ASCII_SET[(n / 7) % N_ASCII]; b[11] = ASCII_SET[(n / 11) % N_ASCII];
                        const uint32_t out = ((n / 4) & 1u) ? 0xFF00Fu : 0u;
                        run_pair(s, pat, b, ((t & 1u) << 7) | ((t & 2u) << 7) | out, 0u, pl, st);
                    }
}

// Every ts4 of BOTH words (256 combinations; bit 0 of the continuation word's is the text-start bit of window index i0 + 4) with the
// text-start bits outside the pair none and all, over a letter, the multiplication sign, an overlong lead and the last two-byte
// character, and four ASCII bytes before and behind, at one place.
void ws_sweep_starts(void* p, int pat, int place, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    const Place& pl = PLACES[place];
    static const uint8_t CH[4][2] = {{0xC3, 0xA9}, {0xC3, 0x97}, {0xC0, 0x80}, {0xDF, 0xBF}};
    static const uint8_t AS[] = {' ', 'a', '7', '\n'};
    for (int c = 0; c < 4; c++)
        for (int x = 0; x < 4; x++)
            for (int y = 0; y < 4; y++)
                for (uint32_t ts8 = 0; ts8 < 256; ts8++)
                    for (uint32_t out = 0; out < 2; out++) {
                        uint8_t b[16];
                        memset(b, 'x', 16);
                        b[6] = AS[x]; b[7] = CH[c][0]; b[8] = CH[c][1]; b[9] = AS[y];
                        run_pair(s, pat, b, (ts8 << 4) | (out ? 0xFF00Fu : 0u), 0u, pl, st);
                    }
}

// Pairs the form must decline by their shape, and the ones it takes among them: the four bytes at the boundary (bytes 2, 3 of the first
// word, 0, 1 of the second) over a small alphabet of ASCII, leads of two-, three- and four-byte characters and continuation bytes, the
// outer bytes of both words ASCII, a continuation byte or a lead; the text-start bits on the two bytes of the boundary; a special-literal
// span on none, on byte 3 or byte 0 of the first word, on byte 0 or byte 3 of the second.
void ws_sweep_shapes(void* p, int pat, int place, uint64_t* st) {
    const Sim& s = *(Sim*)p;
    const Place& pl = PLACES[place];
    static const uint8_t AL[] = {'a', ' ', 0xC3, 0xD0, 0xA9, 0x80, 0xE2, 0xF0, 0xC0};
    static const uint8_t OUTER[] = {'a', 0xA9, 0xC3};
    const int NA = (int)sizeof(AL);
    static const uint32_t SK[] = {0u, 1u << 7, 1u << 4, 1u << 8, 1u << 11};
    for (int code = 0; code < NA * NA * NA * NA; code++)
        for (int o1 = 0; o1 < 3; o1++)
            for (int o2 = 0; o2 < 3; o2++)
                for (uint32_t t = 0; t < 4; t++)
                    for (int sk = 0; sk < 5; sk++) {
                        uint8_t b[16];
                        memset(b, 'x', 16);
                        b[4] = b[5] = OUTER[o1]; b[10] = b[11] = OUTER[o2];
                        for (int k = 0, c = code; k < 4; k++, c /= NA) b[6 + k] = AL[c % NA];
                        run_pair(s, pat, b, (((t & 1u) << 7) | ((t & 2u) << 7)) & ~SK[sk], SK[sk], pl, st);
                    }
}

}  // extern "C"

#ifdef WORDS_STRADDLE_SIM_MAIN
// Stand-alone driver (for a sanitizer build: g++ -fsanitize=address,undefined -DWORDS_STRADDLE_SIM_MAIN ... && ./a.out TABLE):
// every sweep at every place for every pattern; exit status 1 if a sweep is not clean.
int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s unicode_classes.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> u;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) u.insert(u.end(), buf, buf + n);
    fclose(f);
    void* s = ws_create(u.data(), (int)u.size());
    if (!s) { fprintf(stderr, "bad unicode class table\n"); return 2; }
    uint64_t tot[N_STATS] = {0};
    for (int pat = 0; pat < 3; pat++)
        for (int place = 0; place < N_PLACES; place++) {
            uint64_t st[N_STATS] = {0};
            ws_sweep_pairs(s, pat, place, st);
            ws_sweep_starts(s, pat, place, st);
            ws_sweep_shapes(s, pat, place, st);
            for (int k = 0; k < N_STATS; k++) tot[k] += st[k];
        }
    ws_destroy(s);
    printf("cases %llu taken_lead %llu taken_cont %llu inside %llu mismatch %llu declined_wrong %llu took_wrong %llu declined_ts %llu declined_edge %llu declined_shape %llu\n",
           (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2], (unsigned long long)tot[3], (unsigned long long)tot[4],
           (unsigned long long)tot[5], (unsigned long long)tot[6], (unsigned long long)tot[7], (unsigned long long)tot[8], (unsigned long long)tot[9]);
    return (tot[N_MISMATCH] || tot[N_DECLINED_WRONG] || tot[N_TOOK_WRONG]) ? 1 : 0;
}
#endif
