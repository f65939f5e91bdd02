// What the forward-mode point kernels share (k_deform_jet, deform_jet.hip; k_sdf_hessian, sdf_hess.hip).  Such a kernel carries a point
// as a JET: several MLP rows of the lean tile, the value row and its forward tangents, all in ONE lane, so the activation's chain rule
// is between registers.  Written once here: where a point's rows lie, how a lane reaches them, how many points a tile takes, and the
// jet rows of the positional encoding.
//
// Row layout.  The MFMA result has col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): a lane half owns 16 rows of each
// 32-row tile, as four quads.  Those rows, across the tile's row tiles, are the half's SLOTS (slot = 16 ri + reg: 32 on the 64-row
// tile, 16 on the 32-row tile), and point q of a half takes the consecutive slots ROWS q .. ROWS q + ROWS - 1, so every product of its
// rows is between registers of one lane and a quad is still four consecutive rows (lds_store_quad_at as it is).  Slots past the last
// point carry zeros.
#pragma once
#include "chain_common.h"
#include "encode.h"

namespace es {

// the tile row of slot s of lane half hi
__host__ __device__ constexpr int jet_row(int s, int hi) { return 32 * (s >> 4) + 8 * ((s >> 2) & 3) + 4 * hi + (s & 3); }
// and back: the slot of tile row r (its lane half is (r >> 2) & 1)
__host__ __device__ constexpr int jet_slot(int r) { return 16 * (r >> 5) + 4 * ((r >> 3) & 3) + (r & 3); }
// points per lane half and per tile, at ``rows`` MLP rows per point on ``rtc`` row tiles of 32
__host__ __device__ constexpr int jet_pph(int rows, int rtc) { return 16 * rtc / rows; }
__host__ __device__ constexpr int jet_pts(int rows, int rtc) { return 2 * jet_pph(rows, rtc); }

// slot s of n-tile ni in a lane's accumulators (s a constant once the loops around it are unrolled)
template <int RTC>
__device__ __forceinline__ float jet_get(const f32x16 (&acc)[RTC][2], int ni, int s) { return acc[s >> 4][ni][s & 15]; }
template <int RTC>
__device__ __forceinline__ void jet_set(f32x16 (&acc)[RTC][2], int ni, int s, float v) { acc[s >> 4][ni][s & 15] = v; }

constexpr bool jet_slots_are_rows() {          // slot <-> row is a bijection on the 64 rows, for both lane halves
    for (int hi = 0; hi < 2; ++hi)
        for (int s = 0; s < 32; ++s) {
            const int r = jet_row(s, hi);
            if (r < 0 || r >= 64 || ((r >> 2) & 1) != hi || jet_slot(r) != s) return false;
        }
    for (int r = 0; r < 64; ++r)
        if (jet_row(jet_slot(r), (r >> 2) & 1) != r) return false;
    return true;
}
constexpr bool jet_points_fit(int rows, int rtc) {          // every row of every point: in its lane half, inside the tile
    for (int hi = 0; hi < 2; ++hi)
        for (int q = 0; q < jet_pph(rows, rtc); ++q)
            for (int c = 0; c < rows; ++c) {
                const int r = jet_row(rows * q + c, hi);
                if (r >= 32 * rtc || ((r >> 2) & 1) != hi) return false;
            }
    return true;
}
static_assert(jet_slots_are_rows(), "jet_row / jet_slot");
static_assert(jet_points_fit(4, 1) && jet_points_fit(4, 2) && jet_points_fit(8, 1) && jet_points_fit(8, 2) && jet_points_fit(10, 1) &&
                  jet_points_fit(10, 2), "a point's rows stay in one lane half of the tile");
static_assert(jet_pts(4, 1) == 8 && jet_pts(4, 2) == 16 && jet_pts(8, 1) == 4 && jet_pts(8, 2) == 8 && jet_pts(10, 1) == 2 &&
                  jet_pts(10, 2) == 6, "points per tile: Jacobian 8/16, kinematics 4/8, Hessian 2/6");

// One input x at frequency f, entries ks (sin) and kc (cos) of the encoding: the value row r0, the tangent row r1 = d / dx and the
// second row r2 = d2 / dx2.  A kernel that carries no such row passes -1 and nothing is written.
__device__ __forceinline__ void jet_sincos(float* aux, int ks, int kc, float f, float x, int r0, int r1, int r2) {
    float s, co;
    sincosf(x * f, &s, &co);
    aux[swz(ks, r0)] = s;
    aux[swz(kc, r0)] = co;
    if (r1 >= 0) { aux[swz(ks, r1)] = f * co; aux[swz(kc, r1)] = -f * s; }
    if (r2 >= 0) { aux[swz(ks, r2)] = -(f * f) * s; aux[swz(kc, r2)] = -(f * f) * co; }
}

// Work item ``item`` of the encoding jet of tile point p (px [3][64], as encode3 lays the entries out from k = 0): items 0 .. 3 L - 1
// are frequency item / 3 of coordinate item % 3, item 3 L is the identity part.  r0 is the point's value row, tan(c) its tangent row
// along x_c (non-zero in coordinate c's entries only, 1 in its identity entry), sec(c) its second row cc (nothing in the identity
// part) or -1.  The aux rows are zero beforehand; how threads share points and items is the caller's.
template <int L, class Tan, class Sec>
__device__ __forceinline__ void jet_encode3(float* aux, int item, const float* px, int p, int r0, Tan tan, Sec sec) {
    if (item < 3 * L) {
        const int c = item % 3, i = item / 3;
        jet_sincos(aux, enc_index(3, i, 0, c), enc_index(3, i, 1, c), (float)(1 << i), px[c * 64 + p], r0, tan(c), sec(c));
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { aux[swz(c, r0)] = px[c * 64 + p]; aux[swz(c, tan(c))] = 1.f; }
    }
}

// The same for the time t of the point, entries from k = kbase as encode1 lays them out: items 0 .. L - 1 the frequencies, item L the
// identity entry; rt the time tangent's row or -1.
template <int L>
__device__ __forceinline__ void jet_encode1(float* aux, int kbase, int item, float t, int r0, int rt) {
    if (item < L) {
        jet_sincos(aux, kbase + enc_index(1, item, 0, 0), kbase + enc_index(1, item, 1, 0), (float)(1 << item), t, r0, rt, -1);
    } else {
        aux[swz(kbase, r0)] = t;
        if (rt >= 0) aux[swz(kbase, rt)] = 1.f;
    }
}

}  // namespace es
