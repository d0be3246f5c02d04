// tests/native/sim_nw_lcs_masks.cpp -- the two-level match masks of nw_lcs_suffix_kernel (TEST ONLY).
//
// The kernel keeps A[c >> 3] (the columns whose symbol has that high part, and one all-zero pad row) and B[c & 7] in LDS
// and takes M(c) = A[hi(c)] & B[lo(c)]; the layout -- the row count and a code's two byte offsets in one word -- is
// lcs_mask_rows / lcs_mask_offsets of text_alignment_amd/csrc/nw_band.h, the SAME header the kernel compiles.  Here the
// rows are built as the kernel builds them (every column ORs its bit into two rows; a column outside the alphabet ORs 0
// into the pad's), M is compared with the directly built mask of every code, and the bit-parallel row recurrence run on
// these masks, lane by lane with the carry handed up, is compared with a plain dynamic-programming LCS table.
// Built with -DSIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined): the sweep of the Python test,
// exit status 0 iff every case holds.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../text_alignment_amd/csrc/nw_band.h"

using namespace ta;

namespace {

struct Lcg {
    uint64_t x;
    unsigned next() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(x >> 33); }
};

// codes of the alphabet with its last code planted, and every 11th place one of the codes no mask may count
std::vector<int32_t> make_string(int len, int alphabet, Lcg& g) {
    const int32_t outside[4] = {-1, alphabet, alphabet + 1, 255};
    std::vector<int32_t> s(len);
    for (int k = 0; k < len; ++k) s[k] = (int32_t)(g.next() % (unsigned)alphabet);
    for (int k = 5; k < len; k += 11) s[k] = outside[(k / 11) & 3];
    s[(size_t)(g.next() % (unsigned)len)] = alphabet - 1;
    return s;
}

// the rows as the kernel's set-up leaves them: [lcs_mask_rows(alphabet)][64] words; lane l, bit b = reversed column 64 l + b
std::vector<uint64_t> build_rows(const int32_t* o, int m, int alphabet) {
    std::vector<uint64_t> rows((size_t)lcs_mask_rows(alphabet) * 64, 0);
    unsigned char* const base = reinterpret_cast<unsigned char*>(rows.data());
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < 64; ++b) {
            const int c = 64 * lane + b;
            const int sym = c < m ? o[m - 1 - c] : -1;
            const uint32_t off = lcs_mask_offsets(sym, alphabet);
            const uint64_t bit = (unsigned)sym < (unsigned)alphabet ? 1ull << b : 0;
            uint64_t w;
            memcpy(&w, base + (off >> 16) + 8 * lane, 8); w |= bit; memcpy(base + (off >> 16) + 8 * lane, &w, 8);
            memcpy(&w, base + (off & 0xffff) + 8 * lane, 8); w |= bit; memcpy(base + (off & 0xffff) + 8 * lane, &w, 8);
        }
    return rows;
}

// M of a packed pair of offsets at a lane, as a step reads it
uint64_t mask_at(const std::vector<uint64_t>& rows, uint32_t off, int lane) {
    const unsigned char* const base = reinterpret_cast<const unsigned char*>(rows.data());
    const size_t bytes = rows.size() * 8;
    if ((off >> 16) + 8 * lane + 8 > bytes || (off & 0xffff) + 8 * lane + 8 > bytes) return ~0ull;   // (never: check_masks fails on it)
    uint64_t a, b;
    memcpy(&a, base + (off >> 16) + 8 * lane, 8);
    memcpy(&b, base + (off & 0xffff) + 8 * lane, 8);
    return a & b;
}

// 0 if M(code) is the directly built mask for every code of the alphabet and 0 for the pad and the codes outside it
int check_masks(const int32_t* o, int m, int alphabet, int* where) {
    const std::vector<uint64_t> rows = build_rows(o, m, alphabet);
    const int nrows = lcs_mask_rows(alphabet);
    if (nrows != (alphabet + 7) / 8 + 1 + 8) return -1;
    const int codes[5] = {-1, alphabet, alphabet + 1, 255, 1 << 20};
    for (int k = -5; k < alphabet; ++k) {
        const int code = k < 0 ? codes[-k - 1] : k;
        const uint32_t off = k == -5 ? lcs_mask_pad(alphabet) : lcs_mask_offsets(code, alphabet);
        where[0] = code;
        if ((off >> 16) % 512 || (off & 0xffff) % 512 || (int)(off >> 16) / 512 >= nrows || (int)(off & 0xffff) / 512 >= nrows) return -2;
        if (k < 0 && off != lcs_mask_pad(alphabet)) return -3;
        for (int lane = 0; lane < 64; ++lane) {
            uint64_t direct = 0;
            for (int b = 0; b < 64; ++b) {
                const int c = 64 * lane + b;
                if (k >= 0 && c < m && o[m - 1 - c] == code) direct |= 1ull << b;
            }
            where[1] = lane;
            if (mask_at(rows, off, lane) != direct) return k < 0 ? -4 : -5;
        }
    }
    return 0;
}

// 0 if the recurrence V' = (V + (V & M)) | (V & ~M) on the two-level masks, row after row of the reversed strings, gives
// L(i, j) = LCS(t[i..], o[j..]) (a match: equal codes of the alphabet) at every cell: the clear bits among the first
// m - j of row n - i
int check_recurrence(const int32_t* t, int n, const int32_t* o, int m, int alphabet, int* where) {
    const std::vector<uint64_t> rows = build_rows(o, m, alphabet);
    std::vector<int> prev(m + 1, 0), cur(m + 1, 0);                    // the plain table's row i + 1 and row i
    uint64_t V[64];
    for (int l = 0; l < 64; ++l) V[l] = ~0ull;
    for (int i = n - 1; i >= 0; --i) {
        const uint32_t off = lcs_mask_offsets(t[i], alphabet);
        unsigned carry = 0;
        for (int l = 0; l < 64; ++l) {
            const uint64_t M = mask_at(rows, off, l), U = V[l] & M;
            const uint64_t s1 = V[l] + U, s2 = s1 + carry;
            carry = (unsigned)(s1 < V[l]) | (unsigned)(s2 < s1);
            V[l] = s2 | (V[l] & ~M);
        }
        cur[m] = 0;
        for (int j = m - 1; j >= 0; --j) {
            const bool eq = t[i] == o[j] && (unsigned)t[i] < (unsigned)alphabet;
            const int best = prev[j] > cur[j + 1] ? prev[j] : cur[j + 1];
            cur[j] = eq && prev[j + 1] + 1 > best ? prev[j + 1] + 1 : best;
        }
        int count = 0;                                                  // clear bits among the first c = m - j
        for (int c = 0; c <= m; ++c) {
            if (c) count += (int)(~V[(c - 1) >> 6] >> ((c - 1) & 63) & 1);
            where[0] = i; where[1] = m - c;
            if (count != cur[m - c]) return -6;
        }
        for (int c = m; c < 64 * 64; ++c)                               // columns past m: the pad's bit, never a match
            if (!(V[c >> 6] >> (c & 63) & 1)) return -7;
        prev.swap(cur);
    }
    return 0;
}

}  // namespace

// the layout's words for the Python side: rows, the packed offsets of a code, the pad's
extern "C" int sim_lcs_mask_rows(int alphabet) { return lcs_mask_rows(alphabet); }
extern "C" unsigned sim_lcs_mask_offsets(int code, int alphabet) { return lcs_mask_offsets(code, alphabet); }
extern "C" unsigned sim_lcs_mask_pad(int alphabet) { return lcs_mask_pad(alphabet); }
extern "C" long long sim_lcs_mask_lds_bytes(int alphabet, int max_n) { return (long long)lcs_mask_lds_bytes(alphabet, max_n); }
extern "C" int sim_lcs_max_alphabet() { return kLcsMaxAlphabet; }
extern "C" int sim_lcs_max_n() { return kBandMaxLen; }

// the rows of one string as the kernel's set-up builds them, into out[rows x 64] (uint64)
extern "C" int sim_lcs_mask_build(const int32_t* o, int m, int alphabet, uint64_t* out) {
    const std::vector<uint64_t> rows = build_rows(o, m, alphabet);
    memcpy(out, rows.data(), rows.size() * 8);
    return (int)rows.size();
}

// one alphabet and one m: the masks of a seeded string, then the recurrence against the plain table for each listed n;
// the number of checks that held, or a negative code with fail[0..3] = n (0: the masks), and the check's two words
extern "C" int sim_lcs_masks_case(int alphabet, int m, const int* ns, int n_ns, unsigned seed, int* fail) {
    Lcg g{seed * 2654435761ull + (uint64_t)alphabet * 4099 + (uint64_t)m};
    const std::vector<int32_t> o = make_string(m, alphabet, g);
    fail[0] = 0;
    int rc = check_masks(o.data(), m, alphabet, fail + 1);
    if (rc) return rc;
    int held = 1;
    for (int k = 0; k < n_ns; ++k) {
        const std::vector<int32_t> t = make_string(ns[k], alphabet, g);
        fail[0] = ns[k];
        rc = check_recurrence(t.data(), ns[k], o.data(), m, alphabet, fail + 1);
        if (rc) return rc;
        ++held;
    }
    return held;
}

#ifdef SIM_MAIN
#include <cstdio>
int main() {
    const int alphabets[9] = {1, 7, 8, 9, 16, 17, 27, 63, 64}, ms[6] = {1, 63, 64, 65, 4095, 4096}, ns[5] = {2, 63, 64, 65, 257};
    for (int a = 1; a <= kLcsMaxAlphabet; ++a)
        if (lcs_mask_lds_bytes(a, kBandMaxLen) > 10240) { printf("BAD: alphabet %d takes %zu B\n", a, lcs_mask_lds_bytes(a, kBandMaxLen)); return 1; }
    int held = 0;
    for (int a : alphabets)
        for (int m : ms) {
            int fail[3] = {0};
            const int rc = sim_lcs_masks_case(a, m, ns, 5, 7, fail);
            if (rc < 0) { printf("BAD: code %d at alphabet %d m %d n %d (%d %d)\n", rc, a, m, fail[0], fail[1], fail[2]); return 1; }
            held += rc;
        }
    printf("%d checks ok\n", held);
    return 0;
}
#endif
