// The bodies of the GLM training-pass kernels (csrc/bsc_glm.hip's header comment describes the two tile shapes), as
// __device__ templates over the likelihood family F -- a struct of csrc/bsc_families.h, which holds everything a family
// is: nothing here names one -- and compile-time flags, so that several translation units can instantiate them:
//
//   OBS = false   csrc/bsc_glm.hip: glm_pass_kernel / glm_pass_mfma_kernel, the pass over (X, y) alone.  Every use of
//                 the offset and the weight is behind `if (OBS)`, the tile structs carry no extra registers, and the
//                 kernels come out as they did when the bodies lived in that file.
//   OBS = true    csrc/bsc_glm_obs.hip: glm_obs_pass_kernel / glm_obs_pass_mfma_kernel, with a per-row offset o_n
//                 (added to the logit before the link) and a per-row weight v_n >= 0:
//                     l[n,s] = x_n . w_s + o[n],  ell[s] = sum_n v[n] (y[n] l[n,s] - A(l[n,s])),
//                     G[s,:] = sum_n v[n] (y[n] - A'(l[n,s])) x_n
//                 A row with v_n = 0 adds exactly nothing, by a select and not by a product (its link value may have
//                 overflowed).  o and v ride in the tile struct next to y and are loaded the way y is; a null offset
//                 is a zero-record descriptor (reads 0, costs nothing), a null weight a uniform select of 1.0f.
//                 Rows past B read o = 0 and v = 0 through the descriptors.
//   GRP = true    csrc/bsc_glm_group.hip (always with OBS): a per-row group id g_n and one intercept per (group, draw),
//                     l[n,s] = x_n . w_s + Bz[g_n][s] + o[n]
//                 The id rides in the tile next to y (rows past B read id 0); the intercept is gathered through a
//                 descriptor of exactly J * 32 bytes -- no id can read outside the table -- BEFORE the forward
//                 contraction and before the next tile's loads are issued (loads return in order: behind them the
//                 gather would wait for the whole prefetch).  Besides the slab the pass leaves every residual
//                 r_ns = v_n (y_n - A'(l_ns)) in a workspace R, 32 bytes per row in 16-row blocks [block][draw][row],
//                 through a descriptor over what is left of R from the tile's block on: the tail tiles of n_iter run
//                 past the batch and their stores do not land.  Everything of it is behind `if constexpr (GRP)`; the
//                 flag defaults to off and the kernels of the two files above compile as they did without it.
//
//                 GRP with F::SCALAR (csrc/bsc_glm_scalar_group.hip): the slab is the scalar families'; never with ITV.
//
//   F::SCALAR     not a flag: the families with one learned log-scalar per weight draw, tau_s as float32 [S] (always with
//                 OBS; csrc/bsc_glm_nb.hip, csrc/bsc_glm_gamma.hip, csrc/bsc_glm_weibull.hip, csrc/bsc_glm_beta.hip).  A
//                 lane owns ONE draw in both tile shapes, so F::glm_disp's four values are made once per launch and stay
//                 in four registers; T[s] = d ell[s] / d tau_s is one more lane accumulator next to ell.  The slab has no
//                 room for it, so these kernels write block partials of NB_SLAB_STRIDE = REG_SLAB_G + 16 floats: ell at
//                 [SLAB_G + s], T at [SLAB_G + 8 + s].  Everything of it is behind `if constexpr (F::SCALAR)`.
//   ITV = true    csrc/bsc_glm_weibull_interval.hip (a family whose link takes upper ends: Weibull): interval and left
//                 censoring.  One more per-row vector, `upper` [B] float32, rides in the tiles next to y and is loaded
//                 the way y is (rows past B read 0); the family's link says how it is read.  Everything of it is behind
//                 `if constexpr (ITV)`; the flag defaults to off and every other kernel compiles as it did.
//   F::PARAM      not a flag either: a scalar family with one constant per MODEL (csrc/bsc_glm_studentt.hip: the degrees of
//                 freedom).  It is the bodies' last argument `par`, a kernel argument of the scalar_par_* kernels
//                 (csrc/bsc_scalar_family.h), and is read once, by F::glm_disp, which keeps what the link needs of it in
//                 the draw's four registers.  Behind `if constexpr (F::PARAM)`; every other kernel compiles as it did.
//
// Header-only, internal linkage, like csrc/bsc_regress.h.
#pragma once

#include "bsc_families.h"

namespace {

constexpr int SLAB_G = REG_SLAB_G;            // slab[b][d*8 + s], then ell at [SLAB_G + s]
constexpr int SLAB_STRIDE = REG_SLAB_STRIDE;  // floats per block partial
constexpr int NB_SLAB_STRIDE = REG_SLAB_G + 2 * SG;   // F::SCALAR: ell at [SLAB_G + s], T at [SLAB_G + 8 + s]

// ---- 8-row tiles on the VALU (any D % 4 == 0 up to 256): blr_pass_kernel<., 8, .>'s tile (csrc/bsc_regress.h) ----
constexpr int ROWS = 8;
using G8 = Geo<ROWS>;

template <bool OBS, bool GRP = false, bool ITV = false>
struct GlmTile : RowTile<ROWS> {};
template <>
struct GlmTile<true, false, false> : RowTile<ROWS> {
    float ov, vv;   // offset and weight of row lane_value(lane) >> 3, as yv
};
template <>
struct GlmTile<true, false, true> : RowTile<ROWS> {
    float ov, vv;
    float uv;       // ITV: the upper end of the same row (the family's link says how it is read)
};
template <>
struct GlmTile<true, true, false> : RowTile<ROWS> {
    float ov, vv;
    int gv;         // group id of the same row
    float bz;       // Bz[gv][lane_value(lane) & 7], gathered by gather_tile
};

// What the GRP bodies need besides the pass's own arguments (unused, and never touched, without the flag).
struct GlmGroupArgs {
    const int* g;        // [B] group ids, each in [0, J) (checked where the plan is built)
    const float* Bz;     // [J][8]: this launch's chunk of the intercept draws
    int J;
    float* R;            // residuals, [r_blocks][8][16]
    int64_t r_blocks;    // ceil(B / 16)
};
constexpr int R_BLOCK = 16 * SG;   // floats per 16-row block of R

// The intercept table: exactly J records of 32 bytes.  The whole offset of a gather goes into the per-lane operand,
// which is the one the range check covers.
__device__ __forceinline__ auto glm_bz_rsrc(const GlmGroupArgs& ga) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ga.Bz, 0, (unsigned)ga.J * 32u, 0x00020000);
}

// One tile = ROWS rows from row0 on, through descriptors that cover exactly the rows [row0, B).
template <bool FULL, bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void load_tile(GlmTile<OBS, GRP, ITV>& t, const float* __restrict__ X, int64_t ldx,
                                          const float* __restrict__ y, const float* __restrict__ o,
                                          const float* __restrict__ v_, int64_t row0, int64_t B, int D, int lane,
                                          const int* __restrict__ g_ = nullptr,
                                          const float* __restrict__ u_ = nullptr) {
    auto xs = bsc_rows_rsrc(X, ldx, D, B, row0);
    auto ys = bsc_vec_rsrc(y, B, row0);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, 2);   // non-temporal: X is read once
        float4 f = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                               __uint_as_float(v[3]));
        if (!FULL && 4 * lane >= D) f = make_float4(0.f, 0.f, 0.f, 0.f);  // the next row's bytes
        t.x[r] = f;
    }
    t.yv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ys, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
    if constexpr (OBS) {   // a null vector: no records, every lane reads 0
        auto os = bsc_vec_rsrc(o, o ? B : 0, row0);
        auto vs = bsc_vec_rsrc(v_, v_ ? B : 0, row0);
        t.ov = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(os, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
        t.vv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vs, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
    }
    if constexpr (GRP) {
        auto gs = bsc_vec_rsrc(g_, B, row0);
        t.gv = (int)__builtin_amdgcn_raw_buffer_load_b32(gs, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0);
    }
    if constexpr (ITV) {   // rows past B read 0: what y says, and y is dropped there
        auto us = bsc_vec_rsrc(u_, B, row0);
        t.uv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(us, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
    }
}

// GRP: the intercept of this lane's (row, draw), requested before the next tile's loads are issued.
__device__ __forceinline__ void gather_tile(GlmTile<true, true>& t, const GlmGroupArgs& ga, int lane) {
    t.bz = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
        glm_bz_rsrc(ga), 32 * t.gv + 4 * (lane_value<ROWS>(lane) & 7), 0, 0));
}

// Forward + link + backward for one tile; `wl` is this wave's LDS region, `rows_left` = B - row0.  has_v: the weights
// are set (uniform; without them every row weighs 1.0f and real_row alone masks the rows past B).
// GRP: `row0` is the tile's first row (a multiple of 8), its residuals also go to ga.R.
// `dp` is the scalar of this lane's draw, `T` its accumulator (a family without one reads neither).
template <class F, bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void compute_tile(const GlmTile<OBS, GRP, ITV>& t, const float4 (&w)[SG], float4 (&acc)[SG],
                                             float& ell, float* wl, int lane, int64_t rows_left, bool has_v,
                                             const GlmDisp* dp, float* T, const GlmGroupArgs* ga = nullptr,
                                             int64_t row0 = 0) {
    // 1. per-lane partial dots, row by row, into this lane's row of the buffer
    float* mine = wl + lane * G8::PSTR;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        float4 lo, hi;
        lo.x = dot4(t.x[r], w[0]); lo.y = dot4(t.x[r], w[1]);
        lo.z = dot4(t.x[r], w[2]); lo.w = dot4(t.x[r], w[3]);
        hi.x = dot4(t.x[r], w[4]); hi.y = dot4(t.x[r], w[5]);
        hi.z = dot4(t.x[r], w[6]); hi.w = dot4(t.x[r], w[7]);
        *reinterpret_cast<float4*>(mine + r * SG) = lo;
        *reinterpret_cast<float4*>(mine + r * SG + 4) = hi;
    }
    wave_lds_sync();
    // 2. lane k sums values 4g..4g+3 (g = k % 16) over the lane-rows 16 q .. 16 q + 15
    const int g = lane & (G8::NGRP - 1), q = lane / G8::NGRP;
    const float* col = wl + q * G8::RPQ * G8::PSTR + 4 * g;
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int part = 0; part < G8::RPQ / 8; ++part) {
        float4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const float4*>(col + (8 * part + i) * G8::PSTR);
#pragma unroll
        for (int h = 4; h >= 1; h >>= 1) {
#pragma unroll
            for (int i = 0; i < h; ++i) {
                v[i].x += v[i + h].x; v[i].y += v[i + h].y;
                v[i].z += v[i + h].z; v[i].w += v[i + h].w;
            }
        }
        s4.x += v[0].x; s4.y += v[0].y; s4.z += v[0].z; s4.w += v[0].w;
    }
    // 3. fold the row subsets (lane bits 4, 5): lane k ends with the logit of value lane_value(k)
    const float t0 = swap_add32(s4.x, s4.z);
    const float t1 = swap_add32(s4.y, s4.w);
    const float logit = swap_add16(t0, t1);
    const int val = lane_value<ROWS>(lane);
    float l = logit;     // l = logit [+ intercept] [+ offset], then what the tile carries of the row
    if constexpr (GRP) l += t.bz;
    if constexpr (OBS) l += t.ov;
    GlmRow row;
    row.y = t.yv;
    row.real = (int64_t)(val >> 3) < rows_left;
    if constexpr (OBS) row.v = has_v ? t.vv : 1.0f;
    if constexpr (ITV) row.u = t.uv;
    const float resid = glm_link<F, OBS, ITV>(l, row, ell, dp, T);
    if constexpr (GRP) {
        // row row0 + (val >> 3) of block row0 >> 4, draw val & 7; nothing lands from the block r_blocks on
        const int64_t blk = row0 >> 4;
        auto rs = bsc_vec_rsrc(ga->R, ga->r_blocks * R_BLOCK, blk * R_BLOCK);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(resid), rs,
                                              4 * ((val & 7) * 16 + (int)(row0 & 8) + (val >> 3)), 0, 0);
    }
    float* rb = wl + BSC_WAVE * G8::PSTR;
    rb[val] = resid;
    wave_lds_sync();
    // 4. backward: acc[s] += resid(r, s) * x[r]; residuals arrive by LDS broadcast
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (r == 4) asm volatile("" ::: "memory");  // at most four rows of broadcast reads in flight
        const float4 c0 = *reinterpret_cast<const float4*>(rb + r * SG);
        const float4 c1 = *reinterpret_cast<const float4*>(rb + r * SG + 4);
        axpy4(acc[0], c0.x, t.x[r]); axpy4(acc[1], c0.y, t.x[r]);
        axpy4(acc[2], c0.z, t.x[r]); axpy4(acc[3], c0.w, t.x[r]);
        axpy4(acc[4], c1.x, t.x[r]); axpy4(acc[5], c1.y, t.x[r]);
        axpy4(acc[6], c1.z, t.x[r]); axpy4(acc[7], c1.w, t.x[r]);
    }
}

// The block partial: fixed order over the waves, written in slab order [d][s] | ell[s] (| T[s] at NB_SLAB_STRIDE).
template <int STRIDE = SLAB_STRIDE>
__device__ __forceinline__ void write_block_partial(const float* lds, float* __restrict__ slab, int tid) {
    float* out = slab + (int64_t)blockIdx.x * STRIDE;
    for (int i = tid; i < STRIDE; i += PASS_BLOCK) {
        const int src = i < SLAB_G ? (i & 7) * GCOLS + (i >> 3) : i;
        float v = lds[src];
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) v += lds[k * STRIDE + src];
        out[i] = v;
    }
}

// FULL: D == 256.  n_iter: tiles per wave (the same for every wave; tiles past the end read zeros).
// o, v_: the offset and the weight, each may be null; read only where OBS.
// F::SCALAR: logphi [S] (this launch's chunk of the scalar's draws); the slab is NB_SLAB_STRIDE floats per block.
// ITV (a scalar family whose link takes it, without groups): `upper` [B], not null, rides in the tiles next to y.
// F::PARAM: `par`, the family's per-model constant (uniform over the launch), goes to F::glm_disp and nowhere else.
template <class F, bool FULL, bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void glm_pass_body(const float* X, int64_t ldx, const float* y, const float* o,
                                              const float* v_, int64_t B, int D, const float* W, int S, float* slab,
                                              int n_iter, const GlmGroupArgs* ga = nullptr,
                                              const float* logphi = nullptr, const float* upper = nullptr,
                                              float par = 0.f) {
    static_assert(!F::SCALAR || OBS, "the dispersion (the shape) rides with OBS");
    static_assert(!ITV || (F::SCALAR && !GRP), "the upper end rides with a learned shape, without groups");
    constexpr int STRIDE = F::SCALAR ? NB_SLAB_STRIDE : SLAB_STRIDE;
    constexpr int LDS_FLOATS = PASS_WAVES * (G8::WAVE_LDS > STRIDE ? G8::WAVE_LDS : STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wl = lds + wave * G8::WAVE_LDS;
    const bool has_v = OBS && v_ != nullptr;
    GlmDisp dp;          // (dp and tacc: untouched without F::SCALAR)
    float tacc = 0.f;
    if constexpr (F::SCALAR) {   // before anything fills the file
        if constexpr (F::PARAM) dp = F::glm_disp(logphi, lane_value<ROWS>(lane) & 7, S, par);
        else dp = F::glm_disp(logphi, lane_value<ROWS>(lane) & 7, S);
    }

    float4 w[SG], acc[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        w[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * lane < D && s < S) w[s] = *reinterpret_cast<const float4*>(W + (int64_t)s * D + 4 * lane);
        acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float ell = 0.f;

    // This wave owns tiles first, first + stride, ...; every prefetch is unconditional.
    const int64_t stride = (int64_t)gridDim.x * PASS_WAVES;
    int64_t tile = (int64_t)blockIdx.x * PASS_WAVES + wave;
    if constexpr (GRP) {
        // the same rotation; every tile's gather goes out before the loads of the tile after it
        const int* g_ = ga->g;
        GlmTile<OBS, GRP> ta, tb;
        load_tile<FULL, OBS, GRP>(ta, X, ldx, y, o, v_, tile * ROWS, B, D, lane, g_);
        for (int k = 0; k + 1 < n_iter; k += 2) {
            gather_tile(ta, *ga, lane);
            load_tile<FULL, OBS, GRP>(tb, X, ldx, y, o, v_, (tile + stride) * ROWS, B, D, lane, g_);
            compute_tile<F, OBS>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, &dp, &tacc, ga, tile * ROWS);
            gather_tile(tb, *ga, lane);
            load_tile<FULL, OBS, GRP>(ta, X, ldx, y, o, v_, (tile + 2 * stride) * ROWS, B, D, lane, g_);
            compute_tile<F, OBS>(tb, w, acc, ell, wl, lane, B - (tile + stride) * ROWS, has_v, &dp, &tacc, ga,
                                 (tile + stride) * ROWS);
            tile += 2 * stride;
        }
        if (n_iter & 1) {
            gather_tile(ta, *ga, lane);
            compute_tile<F, OBS>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, &dp, &tacc, ga, tile * ROWS);
        }
    } else {
        GlmTile<OBS, false, ITV> ta, tb;
        load_tile<FULL, OBS>(ta, X, ldx, y, o, v_, tile * ROWS, B, D, lane, nullptr, upper);
        for (int k = 0; k + 1 < n_iter; k += 2) {
            load_tile<FULL, OBS>(tb, X, ldx, y, o, v_, (tile + stride) * ROWS, B, D, lane, nullptr, upper);
            compute_tile<F, OBS>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, &dp, &tacc);
            load_tile<FULL, OBS>(ta, X, ldx, y, o, v_, (tile + 2 * stride) * ROWS, B, D, lane, nullptr, upper);
            compute_tile<F, OBS>(tb, w, acc, ell, wl, lane, B - (tile + stride) * ROWS, has_v, &dp, &tacc);
            tile += 2 * stride;
        }
        if (n_iter & 1) compute_tile<F, OBS>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, &dp, &tacc);
    }

    __syncthreads();  // every wave is done with its private region
    float* ep = lds + wave * STRIDE;
#pragma unroll
    for (int s = 0; s < SG; ++s) *reinterpret_cast<float4*>(ep + s * GCOLS + 4 * lane) = acc[s];
    // ell of lane k belongs to draw lane_value(k) & 7; fold the tile rows (lane bits 1 .. 3)
    float ev = ell;
    ev += __shfl_xor(ev, 2);
    ev += __shfl_xor(ev, 4);
    ev += __shfl_xor(ev, 8);
    if ((lane & 14) == 0) ep[SLAB_G + (lane_value<ROWS>(lane) & 7)] = ev;
    if constexpr (F::SCALAR) {   // T folds like ell
        float tv = tacc;
        tv += __shfl_xor(tv, 2);
        tv += __shfl_xor(tv, 4);
        tv += __shfl_xor(tv, 8);
        if ((lane & 14) == 0) ep[SLAB_G + SG + (lane_value<ROWS>(lane) & 7)] = tv;
    }
    __syncthreads();
    write_block_partial<STRIDE>(lds, slab, tid);
}

// ---- 16-row tiles, both contractions on the MFMA pipe (D == 256, y [o, v] 16-byte aligned) ----------------------
constexpr int MT_ROWS = 16;
constexpr int MT_RS = GCOLS + 4;                                // LDS row stride (floats)
constexpr int MT_WAVE_LDS = MT_ROWS * MT_RS + MT_ROWS * SG;     // tile + residuals [draw][row]

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

struct MTileXY {
    float4 x[MT_ROWS];
    float4 yv;     // y[row0 + 4 kq .. + 3]: the rows of this lane's forward result registers
};
template <bool OBS, bool GRP = false, bool ITV = false>
struct MTile : MTileXY {};
template <>
struct MTile<true, false, false> : MTileXY {
    float4 ov, vv;   // offset and weight of the same four rows
};
template <>
struct MTile<true, false, true> : MTileXY {
    float4 ov, vv;
    float4 uv;       // ITV: the upper ends of the same four rows
};
template <>
struct MTile<true, true, false> : MTileXY {
    float4 ov, vv;
    int4 gv;         // group ids of the same four rows
};

__device__ __forceinline__ float4 load_rows4(const float* __restrict__ p, int64_t n, int64_t row0, int lane) {
    auto rs = bsc_vec_rsrc(p, n, row0);
    auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * (lane >> 4), 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

template <bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void load_mtile(MTile<OBS, GRP, ITV>& t, const float* __restrict__ X, int64_t ldx,
                                           const float* __restrict__ y, const float* __restrict__ o,
                                           const float* __restrict__ v_, int64_t row0, int64_t B, int lane,
                                           const int* __restrict__ g_ = nullptr,
                                           const float* __restrict__ u_ = nullptr) {
    auto xs = bsc_rows_rsrc(X, ldx, GCOLS, B, row0);
    auto ys = bsc_vec_rsrc(y, B, row0);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < MT_ROWS; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, 2);   // non-temporal
        t.x[r] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                             __uint_as_float(v[3]));
    }
    auto v = __builtin_amdgcn_raw_buffer_load_b128(ys, 16 * (lane >> 4), 0, 0);
    t.yv = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    if constexpr (OBS) {   // a null vector: no records, every lane reads 0
        t.ov = load_rows4(o, o ? B : 0, row0, lane);
        t.vv = load_rows4(v_, v_ ? B : 0, row0, lane);
    }
    if constexpr (GRP) {
        auto gs = bsc_vec_rsrc(g_, B, row0);
        auto gi = __builtin_amdgcn_raw_buffer_load_b128(gs, 16 * (lane >> 4), 0, 0);
        t.gv = make_int4((int)gi[0], (int)gi[1], (int)gi[2], (int)gi[3]);
    }
    if constexpr (ITV) t.uv = load_rows4(u_, B, row0, lane);
}

template <class F, bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void glm_pass_mfma_body(const float* X, int64_t ldx, const float* y, const float* o,
                                                   const float* v_, int64_t B, const float* W, int S, float* slab,
                                                   int n_iter, const GlmGroupArgs* ga = nullptr,
                                                   const float* logphi = nullptr, const float* upper = nullptr,
                                                   float par = 0.f) {
    static_assert(!F::SCALAR || OBS, "the dispersion (the shape) rides with OBS");
    static_assert(!ITV || (F::SCALAR && !GRP), "the upper end rides with a learned shape, without groups");
    constexpr int STRIDE = F::SCALAR ? NB_SLAB_STRIDE : SLAB_STRIDE;
    constexpr int LDS_FLOATS = PASS_WAVES * (MT_WAVE_LDS > STRIDE ? MT_WAVE_LDS : STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* tl = lds + wave * MT_WAVE_LDS;      // this wave's tile
    float* rb = tl + MT_ROWS * MT_RS;          // residuals [draw][row]
    const bool has_v = OBS && v_ != nullptr;
    GlmDisp dp;
    float tacc = 0.f;
    if constexpr (F::SCALAR) {   // lane (i16, kq) owns draw i16 (live lanes: i16 < 8)
        if constexpr (F::PARAM) dp = F::glm_disp(logphi, i16, S, par);
        else dp = F::glm_disp(logphi, i16, S);
    }

    // forward B operand: W[draw i16][64 kq + 4 j + c]; MFMA columns 8 .. 15 and draws >= S are zero.  Lane group
    // kq contracts columns 64 kq .. 64 kq + 63, which keeps the 16-byte A reads of a lane group conflict-free.
    float wreg[GCOLS / 4];
#pragma unroll
    for (int j = 0; j < GCOLS / 16; ++j) {
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i16 < S) w4 = *reinterpret_cast<const float4*>(W + (int64_t)i16 * GCOLS + 64 * kq + 4 * j);
        wreg[4 * j + 0] = w4.x; wreg[4 * j + 1] = w4.y;
        wreg[4 * j + 2] = w4.z; wreg[4 * j + 3] = w4.w;
    }
    mfma_f32x4 acc[2][4];                      // [draw group][column component]: register i = draw 4 sb + i
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[sb][q] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    float ell = 0.f;
    const bool live = i16 < SG;                // lanes whose forward MFMA column is a draw

    // iteration p of every wave reads one contiguous window of gridDim.x * 4 tiles; p == n_iter: the empty tile
    const int64_t stride0 = (int64_t)gridDim.x * PASS_WAVES;
    const int64_t slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
    auto row0_of = [=](int p) { return p < n_iter ? ((int64_t)p * stride0 + slot) * MT_ROWS : B; };

    const int* g_ = nullptr;
    if constexpr (GRP) g_ = ga->g;
    MTile<OBS, GRP, ITV> t;
    load_mtile<OBS, GRP>(t, X, ldx, y, o, v_, row0_of(0), B, lane, g_, upper);
    for (int p = 0; p < n_iter; ++p) {
        // the tile to LDS, its registers take the next window's tile
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r) *reinterpret_cast<float4*>(tl + r * MT_RS + 4 * lane) = t.x[r];
        const float4 yv = t.yv;
        float4 ov = make_float4(0.f, 0.f, 0.f, 0.f), vv = make_float4(1.f, 1.f, 1.f, 1.f);
        if constexpr (OBS) {   // this tile's offsets and weights, before the prefetch takes the registers
            ov = t.ov;
            if (has_v) vv = t.vv;
        }
        [[maybe_unused]] float4 uv = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (ITV) uv = t.uv;
        const int64_t rows_left = B - row0_of(p) - 4 * kq;     // rows 4 kq + reg < rows_left are real
        float4 bz = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (GRP) {   // the intercepts of this lane's four rows, ahead of the prefetch and of the forward
            auto bs = glm_bz_rsrc(*ga);
            const int so = 4 * (i16 & 7);
            bz.x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.x + so, 0, 0));
            bz.y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.y + so, 0, 0));
            bz.z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.z + so, 0, 0));
            bz.w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.w + so, 0, 0));
        }
        load_mtile<OBS, GRP>(t, X, ldx, y, o, v_, row0_of(p + 1), B, lane, g_, upper);
        wave_lds_sync();

        // forward on v_mfma_f32_16x16x4_f32 (two accumulators: no MFMA waits on its predecessor)
        mfma_f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
        const float* arow = tl + i16 * MT_RS + 64 * kq;
#pragma unroll
        for (int j = 0; j < GCOLS / 16; j += 2) {
            const float4 a0 = *reinterpret_cast<const float4*>(arow + 4 * j);
            const float4 a1 = *reinterpret_cast<const float4*>(arow + 4 * j + 4);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, wreg[4 * j + 0], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, wreg[4 * j + 4], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, wreg[4 * j + 1], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, wreg[4 * j + 5], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, wreg[4 * j + 2], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, wreg[4 * j + 6], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, wreg[4 * j + 3], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, wreg[4 * j + 7], d1, 0, 0, 0);
        }
        // register reg of lane (i16, kq) = logit(row 4 kq + reg, draw i16): the link in the lane, the residuals
        // to rb[draw][row] as one 16-byte store per live lane
        if (live) {
            // row 4 kq + k: l = logit [+ intercept] [+ offset], and what the tile carries of the row.  Both are made
            // HERE and not inside a function around the link: behind one, the compiler moves l's last addition into
            // a link's selects.
            const auto logit = [](float l, float b, float o_) {
                if constexpr (GRP) l += b;
                if constexpr (OBS) l += o_;
                return l;
            };
            const auto row = [](float y_, float v, float u, bool real) {
                GlmRow r;
                r.y = y_;
                r.real = real;
                if constexpr (OBS) r.v = v;
                if constexpr (ITV) r.u = u;
                return r;
            };
            const float r0 = glm_link<F, OBS, ITV>(logit(d0[0] + d1[0], bz.x, ov.x), row(yv.x, vv.x, uv.x, rows_left > 0),
                                                   ell, &dp, &tacc);
            const float r1 = glm_link<F, OBS, ITV>(logit(d0[1] + d1[1], bz.y, ov.y), row(yv.y, vv.y, uv.y, rows_left > 1),
                                                   ell, &dp, &tacc);
            const float r2 = glm_link<F, OBS, ITV>(logit(d0[2] + d1[2], bz.z, ov.z), row(yv.z, vv.z, uv.z, rows_left > 2),
                                                   ell, &dp, &tacc);
            const float r3 = glm_link<F, OBS, ITV>(logit(d0[3] + d1[3], bz.w, ov.w), row(yv.w, vv.w, uv.w, rows_left > 3),
                                                   ell, &dp, &tacc);
            if constexpr (GRP) {
                // block row0 / 16 of R, [draw][row]: nothing lands from the block r_blocks on
                const int64_t blk = row0_of(p) >> 4;
                auto rs = bsc_vec_rsrc(ga->R, ga->r_blocks * R_BLOCK, blk * R_BLOCK);
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                __builtin_amdgcn_raw_buffer_store_b128(
                    u32x4{__float_as_uint(r0), __float_as_uint(r1), __float_as_uint(r2), __float_as_uint(r3)}, rs,
                    4 * (i16 * MT_ROWS + 4 * kq), 0, 0);
            }
            *reinterpret_cast<float4*>(rb + i16 * MT_ROWS + 4 * kq) = make_float4(r0, r1, r2, r3);
        }
        wave_lds_sync();

        // backward on v_mfma_f32_4x4x1_16B_f32: per row two draw groups x four column components
#pragma unroll
        for (int g = 0; g < MT_ROWS / 4; ++g) {
            if (g) asm volatile("" ::: "memory");   // four rows of reads in flight
            float4 ra[2];
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
                ra[sb] = *reinterpret_cast<const float4*>(rb + (4 * sb + (lane & 3)) * MT_ROWS + 4 * g);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float4 x4 = *reinterpret_cast<const float4*>(tl + (4 * g + rr) * MT_RS + 4 * lane);
#pragma unroll
                for (int sb = 0; sb < 2; ++sb) {
                    const float a = rr == 0 ? ra[sb].x : rr == 1 ? ra[sb].y : rr == 2 ? ra[sb].z : ra[sb].w;
                    acc[sb][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.x, acc[sb][0], 0, 0, 0);
                    acc[sb][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.y, acc[sb][1], 0, 0, 0);
                    acc[sb][2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.z, acc[sb][2], 0, 0, 0);
                    acc[sb][3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.w, acc[sb][3], 0, 0, 0);
                }
            }
        }
        wave_lds_sync();   // the next iteration overwrites the tile
    }

    __syncthreads();
    float* ep = lds + wave * STRIDE;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(ep + (4 * sb + i) * GCOLS + 4 * lane) =
                make_float4(acc[sb][0][i], acc[sb][1][i], acc[sb][2][i], acc[sb][3][i]);
    float ev = live ? ell : 0.f;               // lane (i16, kq): rows 4 kq .. of draw i16
    ev += __shfl_xor(ev, 16);
    ev += __shfl_xor(ev, 32);
    if (lane < SG) ep[SLAB_G + lane] = ev;
    if constexpr (F::SCALAR) {
        float tv = live ? tacc : 0.f;
        tv += __shfl_xor(tv, 16);
        tv += __shfl_xor(tv, 32);
        if (lane < SG) ep[SLAB_G + SG + lane] = tv;
    }
    __syncthreads();
    write_block_partial<STRIDE>(lds, slab, tid);
}

// ---- host side ---------------------------------------------------------------------------------------------------

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// 16 = the MFMA kernel (needs the full 256-column layout and 16-byte aligned y, offset, weight, group ids and upper
// ends -- null ones count as aligned), else 8-row tiles.
inline int pass_rows(int D, const float* y, const float* o = nullptr, const float* v = nullptr,
                     const int32_t* g = nullptr, const float* u = nullptr) {
    return (D == GCOLS && aligned16(y) && aligned16(o) && aligned16(v) && aligned16(g) && aligned16(u)) ? MT_ROWS
                                                                                                         : ROWS;
}

// The envelope of the entry points that take an offset and a weight: y by name, the vectors' alignment.
inline int check_glm_obs_args(const char* who, int32_t link, const float* X, int64_t ldx, const float* y, const float* o,
                              const float* v, int64_t B, int32_t D, const float* W, int32_t S, int max_s) {
    BSC_REQUIRE(link == BSC_GLM_LOGISTIC || link == BSC_GLM_POISSON,
                "%s: link=%d must be BSC_GLM_LOGISTIC (0) or BSC_GLM_POISSON (1)", who, link);
    BSC_REQUIRE(y || B <= 0, "%s: y is null with B=%lld", who, (long long)B);
    BSC_REQUIRE((((uintptr_t)o) & 3) == 0 && (((uintptr_t)v) & 3) == 0, "%s: offset and weight must be 4-byte aligned",
                who);
    return check_regress_args(who, X, ldx, B, D, W, S, max_s);
}

// The three kernels of a route: 16-row MFMA tiles, else 8-row tiles with D == 256 (FULL) or any D.  rows8 takes FULL
// as std::true_type / std::false_type, so that the launch site names its 8-row kernel once.
template <class Mfma, class Rows8>
void launch_pass_shape(int rows, int D, Mfma mfma, Rows8 rows8) {
    if (rows == MT_ROWS) mfma();
    else if (D == GCOLS) rows8(std::true_type{});
    else rows8(std::false_type{});
}

// All S draws, eight per launch: pass(s0, sg) launches the pass over draws s0 .. s0 + sg - 1 (timed alone),
// reduce(s0) its slab reduction; tail(s0) is what else the chunk needs (the group sums) and returns a status.
template <class Pass, class Reduce, class Tail>
int for_draw_chunks(bsc_ctx* ctx, int S, Pass pass, Reduce reduce, Tail tail) {
    for (int s0 = 0; s0 < S; s0 += SG) {
        const int sg = S - s0 < SG ? S - s0 : SG;
        {
            bsc_prof_scope prof(ctx);  // times the pass kernel alone
            pass(s0, sg);
        }
        BSC_LAUNCH_CHECK();
        reduce(s0);
        BSC_LAUNCH_CHECK();
        const int rc = tail(s0);
        if (rc != BSC_OK) return rc;
    }
    return BSC_OK;
}

template <class Pass, class Reduce>
int for_draw_chunks(bsc_ctx* ctx, int S, Pass pass, Reduce reduce) {
    return for_draw_chunks(ctx, S, pass, reduce, [](int) { return (int)BSC_OK; });
}

// (The data pass of the scalar families, kernels and host side: csrc/bsc_scalar_family.h.)

}  // namespace

// The launch of the OBS kernels, defined in csrc/bsc_glm_obs.hip and called from csrc/bsc_glm.hip:

// 16-row MFMA tiles when mfma != 0 (D == 256; y and the set ones of o, v 16-byte aligned), else 8-row VALU tiles.
void bsc_glm_obs_launch_pass(bsc_ctx* ctx, int link, int mfma, const float* X, int64_t ldx, const float* y,
                             const float* offset, const float* weight, int64_t B, int D, const float* W, int sg,
                             int n_blocks, int n_iter, float* slab);
