// Ordinal (cumulative-logit, proportional-odds) regression with learned cutpoints on the fused pathwise pass: the data
// pass in the three tile shapes of the GLM routes (csrc/bsc_glm_pass.h: its tiles, loads, grid and draw chunks, with
// bodies of their own below), its slab reduction with the chain rule to the unconstrained cutpoint coordinates, and the
// predictive (csrc/bsc_predict_pass.h's body with its seventh family).  No finish: the latent z = [w (D) | theta (K - 1)]
// has the prior N(0, I / prior_precision) and meets the data through [ell | G], so bsc_glm_update and
// bsc_glm_fullrank_update serve with D := P = D + K - 1, as they serve the softmax route with D := K D.
//
//     y_n in {0 .. K-1},   eta[n,s] = x_n . w_s + o_n,   c_0 < .. < c_{K-2}:   P(y_n <= k) = sigmoid(c_k - eta)
//     theta_0 = c_0,   theta_j = log(c_j - c_{j-1})  (j >= 1): every draw is ordered by construction
// With a = c_{y-1} - eta, b = c_y - eta, U = [y < K-1], L = [y > 0], g = c_y - c_{y-1} and sp the stable softplus:
//     log p          = -U sp(-b) - L sp(a) + U L log(-expm1(-g))            (sigma(b) - sigma(a) without the cancellation)
//     d log p / d eta     = L sigmoid(a) - U sigmoid(-b)                     (the residual that multiplies x_n)
//     d log p / d c_y     = U (sigmoid(-b) + L / expm1(g)),     d log p / d c_{y-1} = -L (sigmoid(a) + U / expm1(g))
// What depends on the draw and the class alone is made ONCE per launch, in float64 and then rounded, into a table in LDS:
// {c_{k-1}, c_k, log(-expm1(-g_k)), 1 / expm1(g_k)} per (draw, class), 8 x 8 x 16 bytes, read with one 16-byte read per
// (row, draw) at the row's label.  The cutpoints are the float32 roundings of the float64 cumulative sum of the float32
// theta the pass read, g the float32 difference of those: the three constants describe exactly the cutpoints the rows
// see.  An end class holds its one cutpoint in both slots and 0 in the other two, so U and L alone switch its terms.
// Per (row, draw) the link is two softplus / sigmoid pairs.  H_j = d ell / d c_j is K - 1 <= 7 lane accumulators, folded
// like ell and written behind it in block partials of ORD_SLAB_STRIDE floats; the chain rule to theta,
//     d ell / d theta_0 = sum_j H_j,     d ell / d theta_i = e^{theta_i} sum_{j >= i} H_j   (i >= 1),
// is parameter-sized and sits in the slab reduction, in float64.
//
// A row is dropped -- adds exactly nothing -- when its weight is 0, when it lies past B, or when its label is outside
// [0, K): by a select on the link's INPUTS (it is evaluated at class 0, eta = 0 and multiplied by an exact 0), so the label
// that indexes the table is always inside it and every int32 value is memory-safe.  The draws Z [S, ldz] need 4-byte
// alignment only (bsc_glm_update writes them [S, P] contiguous and P is in general no multiple of 4): they are read once
// per launch with 4-byte loads.  No float atomics anywhere: the same bits run to run.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_glm_pass.h"
#include "bsc_predict_pass.h"

namespace {

constexpr int MAX_S = 64;
constexpr int ORD_MAX_K = 8;
constexpr int ORD_H = ORD_MAX_K - 1;                          // cutpoints at most
constexpr int ORD_SLAB_STRIDE = REG_SLAB_G + SG + ORD_H * SG;  // ell at [SLAB_G + s], H_j at [SLAB_G + 8 + 8 j + s]
constexpr int ORD_TAB = SG * ORD_MAX_K * 4;                    // floats: [draw][class]{c_{k-1}, c_k, log(-expm1(-g)), 1/expm1(g)}
static_assert(ORD_SLAB_STRIDE % BSC_WAVE == 0, "ell and the H_j are exactly the last workgroup of the slab reduction");

// ---- the per-(draw, class) table: threads 0 .. 63 of the workgroup, once per launch --------------------------------

// Z: this launch's chunk of the draws (theta of draw s at Z[s ldz + D ..]); a dead slot (s >= S) has theta = 0.
__device__ __forceinline__ void ord_build_table(float* tab, const float* __restrict__ Z, int64_t ldz, int D, int K,
                                                int S, int tid) {
    if (tid >= SG * ORD_MAX_K) return;
    const int s = tid >> 3, k = tid & 7;
    double c = 0.0;
    float first = 0.f, lo = 0.f, hi = 0.f, last = 0.f;
    for (int j = 0; j < K - 1; ++j) {
        const float th = s < S ? Z[(int64_t)s * ldz + D + j] : 0.0f;
        c = j == 0 ? (double)th : c + exp((double)th);
        const float cj = (float)c;
        if (j == 0) first = cj;
        if (j == k - 1) lo = cj;
        if (j == k) hi = cj;
        last = cj;
    }
    const bool mid = k >= 1 && k <= K - 2;
    if (k == 0 || k >= K) lo = hi = first;     // (classes from K on are never read)
    else if (k == K - 1) hi = lo = last;
    const double g = (double)(hi - lo);        // the float32 difference of the rounded cutpoints
    float4 t;
    t.x = lo;
    t.y = hi;
    t.z = mid ? (float)log(-expm1(-g)) : 0.0f;
    t.w = mid ? (float)(1.0 / expm1(g)) : 0.0f;
    *reinterpret_cast<float4*>(tab + 4 * tid) = t;
}

// ---- the link --------------------------------------------------------------------------------------------------------

// softplus(x) and sigmoid(x) in the logistic link's forms (csrc/bsc_families.h): finite for every finite x
__device__ __forceinline__ void ord_logistic(float x, float& sp, float& sg) {
    const float e = expf(-fabsf(x));
    const float t = 1.0f + e;
    const float r = __builtin_amdgcn_rcpf(t);
    sg = x >= 0.0f ? r : e * r;
    const float lp = t == 1.0f ? e : __logf(t) * e * __builtin_amdgcn_rcpf(t - 1.0f);
    sp = fmaxf(x, 0.0f) + lp;
}

// `l` already holds the offset, `ybits` the bits of the int32 label, `tabs` this lane's draw's row of the table.
// The selects sit on the INPUTS (csrc/bsc_families.h says why); the H_j take flat selects, one after the other and not nested.
__device__ __forceinline__ float ord_link(float l, float ybits, bool real_row, float vv, const float* tabs, int K,
                                          float& ell, float (&H)[ORD_H]) {
    const int yi = (int)__float_as_uint(ybits);
    const bool keep = real_row && vv > 0.0f && (unsigned)yi < (unsigned)K;
    const float vq = keep ? vv : 0.0f;
    const int yq = keep ? yi : 0;              // what indexes the table is inside it
    const float lq = keep ? l : 0.0f;
    const float4 t = *reinterpret_cast<const float4*>(tabs + 4 * yq);
    const float U = yq < K - 1 ? 1.0f : 0.0f;
    const float L = yq > 0 ? 1.0f : 0.0f;
    float sp_b, sg_b, sp_a, sg_a;
    ord_logistic(lq - t.y, sp_b, sg_b);        // at -b
    ord_logistic(t.x - lq, sp_a, sg_a);        // at a
    ell = fmaf(vq, t.z - fmaf(U, sp_b, L * sp_a), ell);
    const float hu = vq * (U * (sg_b + t.w));  // t.w = 0 unless U = L = 1
    const float hl = -vq * (L * (sg_a + t.w));
#pragma unroll
    for (int j = 0; j < ORD_H; ++j) {
        float d = yq == j + 1 ? hl : 0.0f;
        d = yq == j ? hu : d;
        H[j] += d;
    }
    return vq * fmaf(L, sg_a, -U * sg_b);
}

// ---- 8-row tiles on the VALU: compute_tile of csrc/bsc_glm_pass.h with this link --------------------------------------

__device__ __forceinline__ void ord_compute_tile(const GlmTile<true>& t, const float4 (&w)[SG], float4 (&acc)[SG],
                                                 float& ell, float (&H)[ORD_H], float* wl, const float* tabs, int K,
                                                 int lane, int64_t rows_left, bool has_v) {
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
    // 3. fold the row subsets (lane bits 4, 5): lane k ends with the linear predictor of value lane_value(k)
    const float t0 = swap_add32(s4.x, s4.z);
    const float t1 = swap_add32(s4.y, s4.w);
    const float logit = swap_add16(t0, t1);
    const int val = lane_value<ROWS>(lane);
    const float resid = ord_link(logit + t.ov, t.yv, (int64_t)(val >> 3) < rows_left, has_v ? t.vv : 1.0f, tabs, K,
                                 ell, H);
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

// FULL: D == 256.  y: the int32 labels, read as the float vectors are (their bits are reinterpreted in the link).
// Z [S, ldz]: this launch's chunk of the draws, weights in columns 0 .. D-1, theta behind them; 4-byte loads.
template <bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_ordinal_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v_, int64_t B, int D, int K, const float* __restrict__ Z, int64_t ldz, int S,
    float* __restrict__ slab, int n_iter) {
    constexpr int STRIDE = ORD_SLAB_STRIDE;
    constexpr int LDS_FLOATS = PASS_WAVES * (G8::WAVE_LDS > STRIDE ? G8::WAVE_LDS : STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ __attribute__((aligned(16))) float tab[ORD_TAB];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wl = lds + wave * G8::WAVE_LDS;
    const bool has_v = v_ != nullptr;
    ord_build_table(tab, Z, ldz, D, K, S, tid);     // before anything fills the register file
    const float* tabs = tab + (lane_value<ROWS>(lane) & 7) * (ORD_MAX_K * 4);

    float4 w[SG], acc[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        w[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * lane < D && s < S) {
            const float* zs = Z + (int64_t)s * ldz + 4 * lane;
            w[s] = make_float4(zs[0], zs[1], zs[2], zs[3]);
        }
        acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float ell = 0.f;
    float H[ORD_H];
#pragma unroll
    for (int j = 0; j < ORD_H; ++j) H[j] = 0.f;
    __syncthreads();  // the table

    // This wave owns tiles first, first + stride, ...; every prefetch is unconditional.
    const int64_t stride = (int64_t)gridDim.x * PASS_WAVES;
    int64_t tile = (int64_t)blockIdx.x * PASS_WAVES + wave;
    GlmTile<true> ta, tb;
    load_tile<FULL, true>(ta, X, ldx, y, o, v_, tile * ROWS, B, D, lane);
    for (int k = 0; k + 1 < n_iter; k += 2) {
        load_tile<FULL, true>(tb, X, ldx, y, o, v_, (tile + stride) * ROWS, B, D, lane);
        ord_compute_tile(ta, w, acc, ell, H, wl, tabs, K, lane, B - tile * ROWS, has_v);
        load_tile<FULL, true>(ta, X, ldx, y, o, v_, (tile + 2 * stride) * ROWS, B, D, lane);
        ord_compute_tile(tb, w, acc, ell, H, wl, tabs, K, lane, B - (tile + stride) * ROWS, has_v);
        tile += 2 * stride;
    }
    if (n_iter & 1) ord_compute_tile(ta, w, acc, ell, H, wl, tabs, K, lane, B - tile * ROWS, has_v);

    __syncthreads();  // every wave is done with its private region
    float* ep = lds + wave * STRIDE;
#pragma unroll
    for (int s = 0; s < SG; ++s) *reinterpret_cast<float4*>(ep + s * GCOLS + 4 * lane) = acc[s];
    // ell and H_j of lane k belong to draw lane_value(k) & 7; fold the tile rows (lane bits 1 .. 3)
    const int sd = lane_value<ROWS>(lane) & 7;
    float ev = ell;
    ev += __shfl_xor(ev, 2);
    ev += __shfl_xor(ev, 4);
    ev += __shfl_xor(ev, 8);
    if ((lane & 14) == 0) ep[SLAB_G + sd] = ev;
#pragma unroll
    for (int j = 0; j < ORD_H; ++j) {
        float hv = H[j];
        hv += __shfl_xor(hv, 2);
        hv += __shfl_xor(hv, 4);
        hv += __shfl_xor(hv, 8);
        if ((lane & 14) == 0) ep[SLAB_G + SG + SG * j + sd] = hv;
    }
    __syncthreads();
    write_block_partial<STRIDE>(lds, slab, tid);
}

// ---- 16-row tiles, both contractions on the MFMA pipe: glm_pass_mfma_body of csrc/bsc_glm_pass.h with this link --------

__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_ordinal_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v_, int64_t B, int K, const float* __restrict__ Z, int64_t ldz, int S,
    float* __restrict__ slab, int n_iter) {
    constexpr int STRIDE = ORD_SLAB_STRIDE;
    constexpr int LDS_FLOATS = PASS_WAVES * (MT_WAVE_LDS > STRIDE ? MT_WAVE_LDS : STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ __attribute__((aligned(16))) float tab[ORD_TAB];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* tl = lds + wave * MT_WAVE_LDS;      // this wave's tile
    float* rb = tl + MT_ROWS * MT_RS;          // residuals [draw][row]
    const bool has_v = v_ != nullptr;
    ord_build_table(tab, Z, ldz, GCOLS, K, S, tid);
    const float* tabs = tab + (i16 & 7) * (ORD_MAX_K * 4);   // lane (i16, kq) owns draw i16 (live lanes: i16 < 8)

    // forward B operand: Z[draw i16][64 kq + 4 j + c]; MFMA columns 8 .. 15 and draws >= S are zero
    float wreg[GCOLS / 4];
#pragma unroll
    for (int j = 0; j < GCOLS / 16; ++j) {
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i16 < S) {
            const float* zs = Z + (int64_t)i16 * ldz + 64 * kq + 4 * j;
            w4 = make_float4(zs[0], zs[1], zs[2], zs[3]);
        }
        wreg[4 * j + 0] = w4.x; wreg[4 * j + 1] = w4.y;
        wreg[4 * j + 2] = w4.z; wreg[4 * j + 3] = w4.w;
    }
    mfma_f32x4 acc[2][4];                      // [draw group][column component]: register i = draw 4 sb + i
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[sb][q] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    float ell = 0.f;
    float H[ORD_H];
#pragma unroll
    for (int j = 0; j < ORD_H; ++j) H[j] = 0.f;
    const bool live = i16 < SG;                // lanes whose forward MFMA column is a draw
    __syncthreads();  // the table

    // iteration p of every wave reads one contiguous window of gridDim.x * 4 tiles; p == n_iter: the empty tile
    const int64_t stride0 = (int64_t)gridDim.x * PASS_WAVES;
    const int64_t slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
    auto row0_of = [=](int p) { return p < n_iter ? ((int64_t)p * stride0 + slot) * MT_ROWS : B; };

    MTile<true> t;
    load_mtile<true>(t, X, ldx, y, o, v_, row0_of(0), B, lane);
    for (int p = 0; p < n_iter; ++p) {
        // the tile to LDS, its registers take the next window's tile
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r) *reinterpret_cast<float4*>(tl + r * MT_RS + 4 * lane) = t.x[r];
        const float4 yv = t.yv;
        const float4 ov = t.ov;
        float4 vv = make_float4(1.f, 1.f, 1.f, 1.f);
        if (has_v) vv = t.vv;
        const int64_t rows_left = B - row0_of(p) - 4 * kq;     // rows 4 kq + reg < rows_left are real
        load_mtile<true>(t, X, ldx, y, o, v_, row0_of(p + 1), B, lane);
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
        // register reg of lane (i16, kq) = eta(row 4 kq + reg, draw i16): the link in the lane, the residuals to
        // rb[draw][row] as one 16-byte store per live lane
        if (live) {
            const float r0 = ord_link(d0[0] + d1[0] + ov.x, yv.x, rows_left > 0, vv.x, tabs, K, ell, H);
            const float r1 = ord_link(d0[1] + d1[1] + ov.y, yv.y, rows_left > 1, vv.y, tabs, K, ell, H);
            const float r2 = ord_link(d0[2] + d1[2] + ov.z, yv.z, rows_left > 2, vv.z, tabs, K, ell, H);
            const float r3 = ord_link(d0[3] + d1[3] + ov.w, yv.w, rows_left > 3, vv.w, tabs, K, ell, H);
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
    const float ev = fold4_sum(live ? ell : 0.f);   // lane (i16, kq): rows 4 kq .. of draw i16
    if (lane < SG) ep[SLAB_G + lane] = ev;
#pragma unroll
    for (int j = 0; j < ORD_H; ++j) {
        const float hv = fold4_sum(live ? H[j] : 0.f);
        if (lane < SG) ep[SLAB_G + SG + SG * j + lane] = hv;
    }
    __syncthreads();
    write_block_partial<STRIDE>(lds, slab, tid);
}

// ---- the slab reduction, with the chain rule to theta -------------------------------------------------------------------

// regress_slab_reduce (csrc/bsc_regress.h) at ORD_SLAB_STRIDE, G with row stride P = D + K - 1.  The last workgroup holds
// exactly ell (lanes 0 .. 7) and H_j[s] (lane 8 + 8 j + s): its first wave applies
//     G[s, D]     = sum_j H_j[s],     G[s, D + i] = e^{theta_i} sum_{j >= i} H_j[s]   (i >= 1)
// in float64, the sums from the last cutpoint down.  Z: ALL draws (theta of draw s at Z[s ldz + D ..]).
__global__ __launch_bounds__(RED_BLOCK) void glm_ordinal_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                            int D, int K, int S, int s_base,
                                                                            const float* __restrict__ Z, int64_t ldz,
                                                                            double* __restrict__ ell,
                                                                            double* __restrict__ G) {
    __shared__ double part[RED_WAVES][BSC_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = blockIdx.x * BSC_WAVE + lane;
    const int P = D + K - 1;
    double s4[4];
    slab_run_sum<ORD_SLAB_STRIDE, RED_WAVES>(slab, n_blocks, blockIdx.x * BSC_WAVE, wave, lane, s4, [] {});
    if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[wave][4 * lane + k] = s4[k];
    }
    __syncthreads();
    if (wave != 0) return;
    double tot = part[0][lane];
#pragma unroll
    for (int k = 1; k < RED_WAVES; ++k) tot += part[k][lane];
    if (i < REG_SLAB_G) {
        const int s = i & 7, d = i >> 3;
        if (s_base + s < S && d < D) G[(int64_t)(s_base + s) * P + d] = tot;
        return;
    }
    // (uniform over the workgroup: REG_SLAB_G is a multiple of 64)
    part[0][lane] = tot;
    wave_lds_sync();
    const int s = lane & 7, j = (lane >> 3) - 1;
    if (s_base + s >= S) return;
    if (lane < SG) {
        ell[s_base + s] = tot;
    } else if (j < K - 1) {
        double h = 0.0;
        for (int jj = K - 2; jj >= j; --jj) h += part[0][SG + SG * jj + s];
        if (j >= 1) h *= exp((double)Z[(int64_t)(s_base + s) * ldz + D + j]);
        G[(int64_t)(s_base + s) * P + D + j] = h;
    }
}

// ---- the predictive ---------------------------------------------------------------------------------------------------

// FULL: D == 256.  offset may be null.
template <int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_ordinal_kernel(PredictArgs a, const float* __restrict__ offset,
                                                                     PredictOrdinal od) {
    predict_body<Ordinal, NC, FULL, true>(a, offset, PredictGroups{}, nullptr, od);
}

__global__ __launch_bounds__(BSC_WAVE) void predict_ordinal_sum_kernel(const double* __restrict__ partial, int n,
                                                                       double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int NC>
void launch_predict_ordinal_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const PredictOrdinal& od,
                               int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS)
        hipLaunchKernelGGL((predict_ordinal_kernel<NC, true>), grid, block, 0, ctx->stream, a, offset, od);
    else
        hipLaunchKernelGGL((predict_ordinal_kernel<NC, false>), grid, block, 0, ctx->stream, a, offset, od);
}

// What both entry points ask of K and of the draws.
int check_ordinal_draws(const char* who, int32_t D, int32_t K, const float* Z, int64_t ldz) {
    BSC_REQUIRE(K >= 2 && K <= ORD_MAX_K, "%s: K=%d must be in [2,%d]", who, K, ORD_MAX_K);
    BSC_REQUIRE((((uintptr_t)Z) & 3) == 0, "%s: Z must be 4-byte aligned", who);
    BSC_REQUIRE(ldz >= (int64_t)D + K - 1 && ldz < ((int64_t)1 << 26), "%s: ldz=%lld must be >= D + K - 1 and < 2^26",
                who, (long long)ldz);
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_glm_ordinal_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, const float* offset,
                              const float* weight, int64_t B, int32_t D, int32_t K, const float* Z, int64_t ldz,
                              int32_t S, double* ell, double* G) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_ordinal_data_pass";
    const float* yf = reinterpret_cast<const float*>(y);   // four bytes per row, loaded as the float vectors are
    // the envelope of bsc_glm_data_pass_obs, with the draws' own alignment and leading dimension in the place of W's
    int rc = check_regress_batch(who, X, B, Z);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(y || B <= 0, "%s: y is null with B=%lld", who, (long long)B);
    BSC_REQUIRE((((uintptr_t)y) & 3) == 0 && (((uintptr_t)offset) & 3) == 0 && (((uintptr_t)weight) & 3) == 0,
                "%s: y, offset and weight must be 4-byte aligned", who);
    BSC_REQUIRE(D > 0 && D <= GCOLS && D % 4 == 0, "%s: D=%d must be a multiple of 4 in [4,%d]", who, D, GCOLS);
    BSC_REQUIRE(S >= 1 && S <= MAX_S, "%s: S=%d must be in [1,%d]", who, S, MAX_S);
    BSC_REQUIRE(ldx >= D && ldx % 4 == 0 && ldx < ((int64_t)1 << 26), "%s: ldx=%lld must be >= D, %% 4 == 0 and < 2^26",
                who, (long long)ldx);
    BSC_REQUIRE(((uintptr_t)X & 15) == 0, "%s: X must be 16-byte aligned", who);
    rc = check_ordinal_draws(who, D, K, Z, ldz);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(ell && G, "%s: null output", who);

    const int rows = pass_rows(D, yf, offset, weight);
    const PassGrid g = pass_grid(ctx, B, rows);
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (size_t)g.n_blocks * ORD_SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    float* slab = (float*)ws;
    const dim3 grid(g.n_blocks), block(PASS_BLOCK), rgrid(ORD_SLAB_STRIDE / BSC_WAVE);
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) {   // each launch with its chunk of the draws
            const float* Zs = Z + (int64_t)s0 * ldz;
            launch_pass_shape(
                rows, D,
                [&] {
                    hipLaunchKernelGGL(glm_ordinal_pass_mfma_kernel, grid, block, 0, ctx->stream, X, ldx, yf, offset,
                                       weight, B, (int)K, Zs, ldz, sg, slab, g.n_iter);
                },
                [&](auto full) {
                    hipLaunchKernelGGL(glm_ordinal_pass_kernel<decltype(full)::value>, grid, block, 0, ctx->stream, X,
                                       ldx, yf, offset, weight, B, (int)D, (int)K, Zs, ldz, sg, slab, g.n_iter);
                });
        },
        [&](int s0) {
            hipLaunchKernelGGL(glm_ordinal_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream,
                               (const float*)slab, g.n_blocks, (int)D, (int)K, (int)S, s0, Z, ldz, ell, G);
        });
}

int bsc_ordinal_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, const float* offset,
                             int64_t B, int32_t D, int32_t K, const float* Z, int64_t ldz, int32_t S, float* prob,
                             float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_ordinal_predict_pass";
    const float* yf = reinterpret_cast<const float*>(y);
    int rc = predict_check_batch(who, X, yf, B, Z, prob, nullptr, lpd, lpd_sum);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE((((uintptr_t)y) & 3) == 0 && (((uintptr_t)offset) & 3) == 0, "%s: y and offset must be 4-byte aligned",
                who);
    rc = check_ordinal_draws(who, D, K, Z, ldz);
    if (rc != BSC_OK) return rc;
    PredictArgs a;
    int n_blocks = 0;
    rc = predict_setup(ctx, who, X, ldx, yf, B, D, Z, nullptr, S, prob, nullptr, lpd, lpd_sum, &a, &n_blocks, 3);
    if (rc != BSC_OK || n_blocks == 0) return rc;
    a.mean = nullptr;                     // prob [B, K] travels in PredictOrdinal
    const PredictOrdinal od{prob, ldz, (int)K};
    {
        bsc_prof_scope prof(ctx);
        predict_launch_chunks(S, [&](auto nc) { launch_predict_ordinal_nc<decltype(nc)::value>(ctx, a, offset, od, n_blocks); });
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(predict_ordinal_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream,
                           (const double*)a.partial, n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // extern "C"
