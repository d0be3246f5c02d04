// Host run of the run labeller's building blocks and of the skew-search row arithmetic (text_alignment_amd/csrc/pp_cc.h,
// the header the kernels of ta_preproc.hip compile).  sim_pp_label takes the kernels' steps on one page: the runs of
// every row from 64-pixel segments with the carry (run_starts / run_ends), the tables in raster order, every run joined
// to the touching runs of the row above (join_up, uf_unite_by) inside bands of kRunBand rows first and then across the
// band borders, the roots (uf_root), area and box per root.  tests/test_pp_cc.py holds the component table against
// scipy.ndimage.label and the rows against numpy.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC.
#include <vector>

#include "../../text_alignment_amd/csrc/pp_cc.h"

namespace {

// the ballot of the 64 pixels from column xs on (beyond the row: clear, as pp_run_pixel has it)
unsigned long long ballot(const uint8_t* p, int xs, int w, int want) {
    unsigned long long m = 0;
    for (int lane = 0; lane < 64 && xs + lane < w; ++lane)
        if ((p[xs + lane] != 0) == (want != 0)) m |= 1ull << lane;
    return m;
}

}  // namespace

// Components of the pixels of value `want` (1: ink, 0: paper) of the h x w plane: up to cap records {first pixel in
// raster order, area, x0, y0, x1, y1} in the order of their first pixels; returns their true number, or -1 where the
// starts and the ends of a row's runs do not pair up.
extern "C" int sim_pp_label(const uint8_t* ink, int h, int w, int want, int32_t* recs, int cap) {
    std::vector<int32_t> x0, x1, yrow, row_off(h + 1, 0);
    for (int y = 0; y < h; ++y) {
        const uint8_t* p = ink + (int64_t)y * w;
        row_off[y] = (int32_t)x0.size();
        unsigned long long carry = 0, m = ballot(p, 0, w, want);
        for (int xs = 0; xs < w; xs += 64) {
            const unsigned long long next = ballot(p, xs + 64, w, want);
            const unsigned long long starts = ta::run_starts(m, carry), ends = ta::run_ends(m, next);
            for (int lane = 0; lane < 64; ++lane) {
                if ((starts >> lane) & 1ull) { x0.push_back(xs + lane); yrow.push_back(y); }
                if ((ends >> lane) & 1ull) x1.push_back(xs + lane);
            }
            carry = m >> 63;
            m = next;
        }
        if (x0.size() != x1.size()) return -1;
    }
    const int total = (int)x0.size();
    row_off[h] = total;
    std::vector<int32_t> parent(total);
    for (int i = 0; i < total; ++i) parent[i] = i;
    auto find = [&](int32_t a) { return ta::uf_root(parent.data(), a); };
    for (int borders = 0; borders < 2; ++borders)
        for (int y = 1; y < h; ++y) {
            if ((y % ta::kRunBand == 0) != (borders == 1)) continue;
            for (int i = row_off[y]; i < row_off[y + 1]; ++i)
                ta::join_up(x0.data(), x1.data(), row_off[y - 1], row_off[y], x0[i], x1[i],
                            [&](int j) { ta::uf_unite_by(parent.data(), find, i, j); });
        }
    std::vector<int32_t> area(total, 0), bx0(total, 0x7fffffff), by0(total, 0x7fffffff), bx1(total, -1), by1(total, -1);
    for (int i = 0; i < total; ++i) {
        const int r = find(i);
        area[r] += x1[i] - x0[i] + 1;
        bx0[r] = x0[i] < bx0[r] ? x0[i] : bx0[r]; by0[r] = yrow[i] < by0[r] ? yrow[i] : by0[r];
        bx1[r] = x1[i] > bx1[r] ? x1[i] : bx1[r]; by1[r] = yrow[i] > by1[r] ? yrow[i] : by1[r];
    }
    int count = 0;
    for (int i = 0; i < total; ++i) {
        if (parent[i] != i) continue;
        if (count < cap) {
            int32_t* r = recs + (int64_t)count * 6;
            r[0] = (int32_t)((int64_t)yrow[i] * w + x0[i]); r[1] = area[i];
            r[2] = bx0[i]; r[3] = by0[i]; r[4] = bx1[i]; r[5] = by1[i];
        }
        ++count;
    }
    return count;
}

// rows[k] = the row point (ys[k], xs[k]) of an hs x ws decimated page lands on when the page is turned by the angle of
// cosine ca and sine sa (outside the page included: the kernels drop those afterwards)
extern "C" void sim_pp_skew_rows(const int32_t* ys, const int32_t* xs, int n, int hs, int ws, double ca, double sa, int64_t* rows) {
    const double cy = (hs - 1) / 2.0, cx = (ws - 1) / 2.0;
    for (int k = 0; k < n; ++k) rows[k] = ta::skew_row(ta::skew_t0(ys[k], cy, ca), xs[k], cx, sa);
}
