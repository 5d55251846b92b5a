// fasta_pack.h -- bytes -> slots: check_sequence's tables, the streaming 2-bit packer, the SWAR / AVX2 / AVX-512 fast paths for
// runs of upper-case A/C/G/T, and the ONE walk over a record's sequence lines that every reader goes through:
//   visit_seq_lines   splits a byte range at '\n', skips '#' / '>' lines, strips both ends (bytes.strip()) and hands each line on
//   clean_line        takes a stripped line down the tier ladder (64 / 32 / 16 bases at a time, then byte by byte) into a SINK,
//                     which is what tells the readers apart: count, count + copy, pack, pack + copy, pack + count
// The slot layout is documented in include/idelucs_hip.h.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "dev_env.h"

namespace {

struct Tables {
    uint8_t translate[256];  // utils.py:42-43 basemask; 0 = deleted (" \t\n\r"), 1 = invalid byte
    uint8_t code[256];       // kmers.pyx:19-34: 'A'0 'C'1 'G'2 'T'3, everything else 4
    Tables()
    {
        for (int i = 0; i < 256; ++i) { translate[i] = 1; code[i] = 4; }
        const char *from = "acgtuUswkmyrbdhvnSWKMYRBDHV-";
        const char *to = "ACGTTTNNNNNNNNNNNNNNNNNNNNNN";
        for (const char *c = "ACGTN"; *c; ++c) translate[(uint8_t)*c] = (uint8_t)*c;
        for (int i = 0; from[i]; ++i) translate[(uint8_t)from[i]] = (uint8_t)to[i];
        translate[(uint8_t)' '] = translate[(uint8_t)'\t'] = translate[(uint8_t)'\n'] = translate[(uint8_t)'\r'] = 0;
        code[(uint8_t)'A'] = 0; code[(uint8_t)'C'] = 1; code[(uint8_t)'G'] = 2; code[(uint8_t)'T'] = 3;
    }
};
const Tables T;

inline bool py_bytes_space(uint8_t b) { return b == ' ' || (b >= 9 && b <= 13); }  // bytes.strip() set

// streaming 2-bit packer (first base in the top pair of each word; invalid-mask bit 31-j per base)
struct Packer {
    uint32_t *cw, *mw;
    uint32_t c = 0, m = 0;
    int j = 0;
    int64_t w = 0;
    bool dirty = false;                // an invalid base (N) was pushed: the record's mask is more than its tail padding
    inline void push(unsigned code)
    {
        if (code == 4u) { m |= 0x8000u >> j; dirty = true; }
        else c |= (uint32_t)code << (30 - 2 * j);
        if (++j == 16) flush_word();
    }
    inline void flush_word()
    {
        cw[w] = c;
        if ((w & 1) == 0) mw[w >> 1] = m << 16; else mw[w >> 1] |= m;
        ++w; c = 0; m = 0; j = 0;
    }
    inline void clean_word(uint32_t codes) { c = codes; m = 0; j = 16; flush_word(); }      // 16 valid bases at a word boundary
    inline void clean_words(int64_t n)         // at a word boundary, n code words of valid bases have been stored at cw + w: their mask bits
    {
        const int64_t m0 = (w + 1) >> 1, m1 = (w + n + 1) >> 1;      // the mask words that BEGIN in [w, w + n) (an odd w's word keeps its first half)
        memset(mw + m0, 0, (size_t)(m1 - m0) * sizeof(uint32_t));
        w += n;
    }
    void finish(int64_t slots)
    {
        if (j > 0) { for (int t = j; t < 16; ++t) m |= 0x8000u >> t; j = 16; flush_word(); }
        while (w < slots * 4) { c = 0; m = 0xFFFFu; flush_word(); }
    }
};

enum { REC_OK = 0, REC_BAD_HEADER = 1, REC_TAB = 2, REC_BAD_BASE = 3 };

// ---- eight bases at a time (SWAR): the overwhelmingly common input is runs of upper-case A/C/G/T, for which neither the
// translate table nor the per-base packer is needed.  Anything else falls back to the byte loop of clean_line, so the result is the same.
inline uint64_t load8(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }      // byte 0 = first base (little endian)

inline bool all_acgt8(uint64_t x)
{
    auto zero_bytes = [](uint64_t v) { const uint64_t L = 0x7F7F7F7F7F7F7F7FULL; return ~(((v & L) + L) | v | L); };               // exact: 0x80 in every byte of v that is 0
    const uint64_t hit = zero_bytes(x ^ 0x4141414141414141ULL) | zero_bytes(x ^ 0x4343434343434343ULL) |
                         zero_bytes(x ^ 0x4747474747474747ULL) | zero_bytes(x ^ 0x5454545454545454ULL);
    return hit == 0x8080808080808080ULL;
}

inline uint32_t pack8(uint64_t x)           // 8 valid bases -> 16 bits, first base in the top pair, A0 C1 G2 T3
{
    uint64_t c = (x >> 1) & 0x0303030303030303ULL;                    // A0 C1 G3 T2
    c ^= (c >> 1) & 0x0101010101010101ULL;                            // A0 C1 G2 T3
    const uint64_t M = (1ull << 30) | (1ull << 20) | (1ull << 10) | 1ull;  // byte i of a 4-byte group -> bit pair 30 - 2 i (no two terms overlap)
    const uint32_t p0 = (uint32_t)(((uint64_t)(uint32_t)c * M) >> 24) & 0xFFu;
    const uint32_t p1 = (uint32_t)(((uint64_t)(uint32_t)(c >> 32) * M) >> 24) & 0xFFu;
    return (p0 << 8) | p1;
}

// ---- the same with AVX2 where the host has it (runtime dispatch; the SWAR code above is the portable path)
#if defined(__x86_64__)
#define IDL_HAVE_AVX2_PATH 1
inline bool host_has_avx2() { static const bool h = __builtin_cpu_supports("avx2"); return h; }

__attribute__((target("avx2"))) inline bool all_acgt32_avx2(const uint8_t *p)
{
    const __m256i v = _mm256_loadu_si256((const __m256i *)p);
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, _mm256_set1_epi8('A')), _mm256_cmpeq_epi8(v, _mm256_set1_epi8('C'))),
                                       _mm256_or_si256(_mm256_cmpeq_epi8(v, _mm256_set1_epi8('G')), _mm256_cmpeq_epi8(v, _mm256_set1_epi8('T'))));
    return (uint32_t)_mm256_movemask_epi8(ok) == 0xFFFFFFFFu;
}

// 32 valid bases -> two code words (16 bases each, first base in the top pair, A0 C1 G2 T3)
__attribute__((target("avx2"))) inline void pack32_avx2(const uint8_t *p, uint32_t *w)
{
    const __m256i v = _mm256_loadu_si256((const __m256i *)p);
    __m256i c = _mm256_and_si256(_mm256_srli_epi16(v, 1), _mm256_set1_epi8(3));                  // A0 C1 G3 T2
    c = _mm256_xor_si256(c, _mm256_and_si256(_mm256_srli_epi16(c, 1), _mm256_set1_epi8(1)));     // A0 C1 G2 T3
    const __m256i p2 = _mm256_maddubs_epi16(c, _mm256_set1_epi16(0x0104));      // bytes (b0, b1) -> b0 * 4 + b1 in a 16-bit lane
    const __m256i p4 = _mm256_madd_epi16(p2, _mm256_set1_epi32(0x00010010));     // 16-bit (q0, q1) -> q0 * 16 + q1 in a 32-bit lane: 4 bases, first on top
    // the low byte of each 32-bit lane is one packed byte; a word wants its 4 bytes with the FIRST one most significant
    const __m256i sh = _mm256_setr_epi8(12, 8, 4, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                        12, 8, 4, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    const __m256i g = _mm256_shuffle_epi8(p4, sh);
    w[0] = (uint32_t)_mm256_extract_epi32(g, 0);
    w[1] = (uint32_t)_mm256_extract_epi32(g, 4);
}

// ---- and with AVX-512 a whole slot at a time: 64 valid bases -> the slot's four code words in one 16-byte store
inline bool host_has_avx512() { static const bool h = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw"); return h; }

__attribute__((target("avx512f,avx512bw"))) inline bool pack64_avx512(const uint8_t *p, uint32_t *w4)
{
    const __m512i v = _mm512_loadu_si512((const void *)p);
    const __mmask64 ok = _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8('A')) | _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8('C')) |
                         _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8('G')) | _mm512_cmpeq_epi8_mask(v, _mm512_set1_epi8('T'));
    if (ok != ~(__mmask64)0) return false;
    __m512i c = _mm512_and_si512(_mm512_srli_epi16(v, 1), _mm512_set1_epi8(3));                  // A0 C1 G3 T2
    c = _mm512_xor_si512(c, _mm512_and_si512(_mm512_srli_epi16(c, 1), _mm512_set1_epi8(1)));     // A0 C1 G2 T3
    const __m512i p2 = _mm512_maddubs_epi16(c, _mm512_set1_epi16(0x0104));      // bytes (b0, b1) -> b0 * 4 + b1
    const __m512i p4 = _mm512_madd_epi16(p2, _mm512_set1_epi32(0x00010010));     // (q0, q1) -> q0 * 16 + q1: 4 bases per 32-bit lane, first on top
    // per 128-bit lane: the low bytes of its four 32-bit lanes, the FIRST most significant, into its first dword; then the four dwords together
    const __m512i sh = _mm512_broadcast_i32x4(_mm_setr_epi8(12, 8, 4, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1));
    const __m512i g = _mm512_shuffle_epi8(p4, sh);
    const __m512i idx = _mm512_setr_epi32(0, 4, 8, 12, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    _mm_storeu_si128((__m128i *)w4, _mm512_castsi512_si128(_mm512_permutexvar_epi32(idx, g)));
    return true;
}

// memchr(p, '\n', n) for the one-pass reader's long sequence lines, with a software prefetch ahead of the scan: the hardware
// prefetchers stop at every 4 KB page, so a thread streaming a mapping of the page cache takes one full memory latency per page
// (IDELUCS_DEV=prefetch = bytes ahead, default 2048; 0 = plain memchr).  The scan is the first touch of the line; the packer behind
// it reads the cache.
__attribute__((target("avx512f,avx512bw"))) inline const uint8_t *find_nl_avx512(const uint8_t *p, size_t n, size_t ahead)
{
    const __m512i nl = _mm512_set1_epi8('\n');
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        _mm_prefetch((const char *)(p + i + ahead), _MM_HINT_T0);
        const __mmask64 m = _mm512_cmpeq_epi8_mask(_mm512_loadu_si512((const void *)(p + i)), nl);
        if (m) return p + i + __builtin_ctzll(m);
    }
    return i < n ? (const uint8_t *)memchr(p + i, '\n', n - i) : nullptr;
}
inline const uint8_t *find_nl(const uint8_t *p, size_t n)
{
    static const size_t ahead = [] { const char *e = idl::dev_env("prefetch"); const long v = e ? atol(e) : 2048; return (size_t)(v < 0 ? 0 : (v > 65536 ? 65536 : v)); }();
    if (ahead != 0 && n >= 256 && host_has_avx512()) return find_nl_avx512(p, n, ahead);
    return (const uint8_t *)memchr(p, '\n', n);
}

// the two wide tiers of clean_line: the number of leading 64- / 32-base blocks of [a, b) that are pure upper-case A/C/G/T, their
// code words stored back to back from cw (PACK).  (The loops live in functions of the tier's own target, so that test and pack are
// inlined into one loop; they see no sink, so that the sink and its packer stay in registers around the call.)
__attribute__((target("avx512f,avx512bw"))) inline int64_t run64_avx512(const uint8_t *a, const uint8_t *b, uint32_t *cw)
{
    int64_t k = 0;
    while (b - a >= 64 && pack64_avx512(a, cw + 4 * k)) { a += 64; ++k; }
    return k;
}
template <bool PACK>
__attribute__((target("avx2"))) inline int64_t run32_avx2(const uint8_t *a, const uint8_t *b, uint32_t *cw)
{
    int64_t k = 0;
    while (b - a >= 32 && all_acgt32_avx2(a)) {
        if constexpr (PACK) pack32_avx2(a, cw + 2 * k);
        a += 32; ++k;
    }
    return k;
}
#else
#define IDL_HAVE_AVX2_PATH 0
inline const uint8_t *find_nl(const uint8_t *p, size_t n) { return (const uint8_t *)memchr(p, '\n', n); }
#endif

// ---- the sink: what becomes of the cleaned bases of a line, by three switches.
//   PACK     2-bit pack through pk (the sink's own, by value: the hot loops keep it in registers; the caller finishes the record
//            through it).  A packing sink has word alignment to respect, takes the 64-base tier, and its SWAR step is a whole
//            16-base code word; without PACK nothing is aligned and the step is 8.
//   COPY     write the cleaned bases to dst
//   CHECKED  count them, and end the walk with REC_BAD_BASE at an INVALID byte; otherwise invalid bytes are skipped.  That policy is
//            chosen where the sink is instantiated (host_ingest.cpp: pack_record, one_pass_slice).
template <bool PACK, bool COPY, bool CHECKED>
struct Sink {
    static constexpr bool PACKS = PACK, REPORTS = CHECKED;
    static constexpr int SWAR = PACK ? 16 : 8;
    Packer pk;
    uint8_t *dst = nullptr;
    int64_t cnt = 0;
    inline bool at_word() const { return !PACK || pk.j == 0; }
    inline bool at_slot() const { return PACK && pk.j == 0 && (pk.w & 3) == 0; }
    inline int to_word() const { return PACK ? 16 - pk.j : SWAR; }
    inline uint32_t *code_words() const { return PACK ? pk.cw + pk.w : nullptr; }
    inline void took(const uint8_t *a, int64_t n)         // n clean bases at a, already packed
    {
        if constexpr (COPY) { memcpy(dst, a, (size_t)n); dst += n; }
        if constexpr (CHECKED) cnt += n;
    }
    inline void took_wide(const uint8_t *a, int64_t n)    // (a wide tier has stored their code words at code_words())
    {
        if constexpr (PACK) pk.clean_words(n / 16);
        took(a, n);
    }
    inline void take_swar(const uint8_t *a, uint64_t x0, uint64_t x1)
    {
        if constexpr (PACK) pk.clean_word((pack8(x0) << 16) | pack8(x1));
        took(a, SWAR);
    }
    inline void base(uint8_t t)
    {
        if constexpr (COPY) *dst++ = t;
        if constexpr (PACK) pk.push(T.code[t]);
        if constexpr (CHECKED) ++cnt;
    }
};
using CountSink = Sink<false, false, true>;          // validate + count
using CopySink = Sink<false, true, true>;            // ... + the cleaned bytes
using PackOnlySink = Sink<true, false, false>;       // pack a record that was validated before
using PackCopySink = Sink<true, true, false>;        // ... + the cleaned bytes
using PackCheckedSink = Sink<true, false, true>;     // validate + count + pack in one go

// One stripped sequence line [a, b) into a sink: translate + delete (check_sequence, utils.py:42-51), clean runs by the widest
// tier that fits -- 64 bases at a slot boundary with AVX-512, 32 with AVX2, the sink's SWAR step with 8-byte loads -- and byte by
// byte up to the next word boundary around anything else.  REC_BAD_BASE with *bad = the byte when a reporting sink meets an invalid one.
template <typename Sink>
inline int clean_line(const uint8_t *a, const uint8_t *b, Sink &s, uint8_t *bad)
{
    while (a < b) {
#if IDL_HAVE_AVX2_PATH
        if constexpr (Sink::PACKS) {
            if (s.at_slot() && b - a >= 64 && host_has_avx512()) {      // whole slots
                const int64_t n = 64 * run64_avx512(a, b, s.code_words());
                s.took_wide(a, n); a += n;
                if (a >= b) break;
            }
        }
        if (s.at_word() && b - a >= 32 && host_has_avx2()) {
            const int64_t n = 32 * run32_avx2<Sink::PACKS>(a, b, s.code_words());
            s.took_wide(a, n); a += n;
            if (a >= b) break;
        }
#endif
        if (s.at_word() && b - a >= Sink::SWAR) {
            const uint64_t x0 = load8(a), x1 = Sink::SWAR == 16 ? load8(a + 8) : x0;
            if (all_acgt8(x0) && all_acgt8(x1)) { s.take_swar(a, x0, x1); a += Sink::SWAR; continue; }
        }
        const int64_t room = s.at_word() ? Sink::SWAR : s.to_word();      // to the next point at which a tier may start again
        const uint8_t *stop = b - a > room ? a + room : b;
        for (; a < stop; ++a) {
            const uint8_t t = T.translate[*a];
            if (t == 0) continue;
            if (t == 1) {
                if constexpr (Sink::REPORTS) { *bad = *a; return REC_BAD_BASE; }
                else continue;
            }
            s.base(t);
        }
    }
    return REC_OK;
}

// newline finders for visit_seq_lines
struct MemchrNl { inline const uint8_t *operator()(const uint8_t *p, size_t n) const { return (const uint8_t *)memchr(p, '\n', n); } };
struct PrefetchNl { inline const uint8_t *operator()(const uint8_t *p, size_t n) const { return find_nl(p, n); } };

// The sequence lines of [p, end), the reference's way (utils.py:137-188): split at '\n', lines that begin with '#' or '>' skipped,
// the others .strip()ped at both ends and handed to line(a, b), whose non-zero return ends the walk and is returned.  stop(first
// byte of a line) ends it before that line (the one-pass reader: the next '>' line; the general reader knows its range: never).
// p is left at the line the walk ended on.
template <typename FindNl, typename Stop, typename Line>
inline int visit_seq_lines(const uint8_t *&p, const uint8_t *end, FindNl find, Stop stop, Line line)
{
    while (p < end && !stop(*p)) {
        const uint8_t *nl = find(p, (size_t)(end - p));
        const uint8_t *le = nl ? nl + 1 : end;
        if (*p != '#' && *p != '>') {
            const uint8_t *a = p, *b = le;
            while (a < b && py_bytes_space(*a)) ++a;
            while (b > a && py_bytes_space(b[-1])) --b;
            if (const int rc = line(a, b)) return rc;
        }
        p = le;
    }
    return 0;
}

// a record's data range [p, end) of the general reader through clean_line into a sink / raw (check == 0: no translate) byte by byte
template <typename Sink>
inline int clean_range(const uint8_t *p, const uint8_t *end, Sink &s, uint8_t *bad)
{
    return visit_seq_lines(p, end, MemchrNl(), [](uint8_t) { return false; }, [&](const uint8_t *a, const uint8_t *b) { return clean_line(a, b, s, bad); });
}
template <typename Emit>
inline void raw_range(const uint8_t *p, const uint8_t *end, Emit emit)
{
    (void)visit_seq_lines(p, end, MemchrNl(), [](uint8_t) { return false; }, [&](const uint8_t *a, const uint8_t *b) { for (; a < b; ++a) emit(*a); return 0; });
}

}  // namespace
