// Reparameterised SVI for canonical-link GLMs: Bernoulli-logit and Poisson-log regression.
//
// ABSENT in the reference: README.md:51 (reparameterisation trick, refs [10][11][12]) and README.md:69-79
// (mini-batch SVI) on the likelihood split of bayesic/distribution/base.py:47-69, for the two non-conjugate
// likelihoods people use VI for.  With l_ns = x_n . w_s the data-sized work of one update is
//     ell[s]  = sum_n [y_n l_ns - A(l_ns)]
//     G[s, :] = sum_n (y_n - A'(l_ns)) x_n
// A = softplus (logistic), A = exp (Poisson): the shape of csrc/bsc_blr.hip's pass with another per-row
// function, so the kernels below are that file's -- one read of X[B, D] and y[B] for up to eight draws, the same
// tiles, the same slab of per-workgroup partials ([d * 8 + s] then eight scalars, ell where BLR keeps Q) and
// the same float64 fixed-order reduction (no float atomics: bitwise reproducible).
//
//   D == 256   glm_pass_mfma_kernel: a wave owns 16-row tiles, prefetched through registers (non-temporal
//              buffer loads: X is read once) and parked row-major in the wave's LDS region.  Forward on
//              v_mfma_f32_16x16x4_f32 with W as the B operand: lane (draw = lane % 16, kq = lane / 16) ends with
//              the logits of rows 4 kq .. 4 kq + 3 of its draw in four registers, applies the link to them in
//              place and hands the residuals y - A'(l) to the backward through LDS ([draw][row]).  Backward:
//              the rank-1 updates G[s, :] += r[n, s] x[n, :] on v_mfma_f32_4x4x1_16B_f32 into per-lane
//              accumulators (register i of accumulator (sb, q) = G[4 sb + i][4 lane + q]).
//   otherwise  glm_pass_kernel: 8-row tiles, lane l holds columns 4 l .. 4 l + 3 of every row, the 64 partial
//              dot products of a lane are transposed and summed through the wave's LDS region, the link runs on
//              one (row, draw) per lane, the residuals come back by LDS broadcast.
//
// Rows past the end of the mini-batch read as zeros through the buffer descriptor (no ragged-tail path); their
// logit is 0, so they add nothing to G (x = 0) and are masked out of ell (A(0) != 0).
#include "bsc_regress.h"

namespace {

constexpr int SLAB_G = REG_SLAB_G;            // slab[b][d*8 + s], then ell at [SLAB_G + s]
constexpr int SLAB_STRIDE = REG_SLAB_STRIDE;  // floats per block partial
constexpr int MAX_S = 64;

// ---- the link: ell += y l - A(l) for a real row, resid = y - A'(l) ------------------------------------------
//
// Logistic: A = softplus in the stable form max(l, 0) + log1p(e), e = exp(-|l|) <= 1 (exp at full float32 accuracy:
// the tails at |l| = 80 are compared at rtol 1e-6), and A' = sigmoid from the
// same e (1 / (1 + e) for l >= 0, e / (1 + e) below): finite for every finite l.  Poisson: A = A' = exp(l),
// NOT clamped (a clamp would change the gradient silently): finite for l <= 88.
template <int LINK>
__device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell) {
    float a, da;
    if (LINK == BSC_GLM_LOGISTIC) {
        const float e = expf(-fabsf(l));
        const float t = 1.0f + e;
        const float r = __builtin_amdgcn_rcpf(t);
        da = l >= 0.0f ? r : e * r;
        // log1p(e) = log(t) e / (t - 1): the quotient undoes the rounding of t = 1 + e (t - 1 is exact); t == 1: e itself.
        // Within 3e-7 of log1p over e in [0, 1], ten vector instructions where the library's log1pf is ~90.
        const float lp = t == 1.0f ? e : __logf(t) * e * __builtin_amdgcn_rcpf(t - 1.0f);
        a = fmaxf(l, 0.0f) + lp;
    } else {
        a = expf(l);
        da = a;
    }
    ell += real_row ? fmaf(yv, l, -a) : 0.0f;
    return yv - da;
}

// ---- 8-row tiles on the VALU (any D % 4 == 0 up to 256): blr_pass_kernel<., 8, .>'s tile (csrc/bsc_regress.h) ----
constexpr int ROWS = 8;
using G8 = Geo<ROWS>;
using Tile = RowTile<ROWS>;

// One tile = ROWS rows from row0 on, through descriptors that cover exactly the rows [row0, B).
template <bool FULL>
__device__ __forceinline__ void load_tile(Tile& t, const float* __restrict__ X, int64_t ldx,
                                          const float* __restrict__ y, int64_t row0, int64_t B, int D, int lane) {
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
}

// Forward + link + backward for one tile; `wl` is this wave's LDS region, `rows_left` = B - row0.
template <int LINK>
__device__ __forceinline__ void compute_tile(const Tile& t, const float4 (&w)[SG], float4 (&acc)[SG], float& ell,
                                             float* wl, int lane, int64_t rows_left) {
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
    const float resid = glm_link<LINK>(logit, t.yv, (int64_t)(val >> 3) < rows_left, ell);
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

// The block partial: fixed order over the waves, written in slab order [d][s] | ell[s].
__device__ __forceinline__ void write_block_partial(const float* lds, float* __restrict__ slab, int tid) {
    float* out = slab + (int64_t)blockIdx.x * SLAB_STRIDE;
    for (int i = tid; i < SLAB_STRIDE; i += PASS_BLOCK) {
        const int src = i < SLAB_G ? (i & 7) * GCOLS + (i >> 3) : i;
        float v = lds[src];
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) v += lds[k * SLAB_STRIDE + src];
        out[i] = v;
    }
}

// FULL: D == 256.  n_iter: tiles per wave (the same for every wave; tiles past the end read zeros).
template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B, int D,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter) {
    constexpr int LDS_FLOATS = PASS_WAVES * (G8::WAVE_LDS > SLAB_STRIDE ? G8::WAVE_LDS : SLAB_STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wl = lds + wave * G8::WAVE_LDS;

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
    Tile ta, tb;
    load_tile<FULL>(ta, X, ldx, y, tile * ROWS, B, D, lane);
    for (int k = 0; k + 1 < n_iter; k += 2) {
        load_tile<FULL>(tb, X, ldx, y, (tile + stride) * ROWS, B, D, lane);
        compute_tile<LINK>(ta, w, acc, ell, wl, lane, B - tile * ROWS);
        load_tile<FULL>(ta, X, ldx, y, (tile + 2 * stride) * ROWS, B, D, lane);
        compute_tile<LINK>(tb, w, acc, ell, wl, lane, B - (tile + stride) * ROWS);
        tile += 2 * stride;
    }
    if (n_iter & 1) compute_tile<LINK>(ta, w, acc, ell, wl, lane, B - tile * ROWS);

    __syncthreads();  // every wave is done with its private region
    float* ep = lds + wave * SLAB_STRIDE;
#pragma unroll
    for (int s = 0; s < SG; ++s) *reinterpret_cast<float4*>(ep + s * GCOLS + 4 * lane) = acc[s];
    // ell of lane k belongs to draw lane_value(k) & 7; fold the tile rows (lane bits 1 .. 3)
    float ev = ell;
    ev += __shfl_xor(ev, 2);
    ev += __shfl_xor(ev, 4);
    ev += __shfl_xor(ev, 8);
    if ((lane & 14) == 0) ep[SLAB_G + (lane_value<ROWS>(lane) & 7)] = ev;
    __syncthreads();
    write_block_partial(lds, slab, tid);
}

// ---- 16-row tiles, both contractions on the MFMA pipe (D == 256, y 16-byte aligned) ---------------------------
constexpr int MT_ROWS = 16;
constexpr int MT_RS = GCOLS + 4;                                // LDS row stride (floats)
constexpr int MT_WAVE_LDS = MT_ROWS * MT_RS + MT_ROWS * SG;     // tile + residuals [draw][row]

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

struct MTile {
    float4 x[MT_ROWS];
    float4 yv;     // y[row0 + 4 kq .. + 3]: the rows of this lane's forward result registers
};

__device__ __forceinline__ void load_mtile(MTile& t, const float* __restrict__ X, int64_t ldx,
                                           const float* __restrict__ y, int64_t row0, int64_t B, int lane) {
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
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter) {
    constexpr int LDS_FLOATS = PASS_WAVES * (MT_WAVE_LDS > SLAB_STRIDE ? MT_WAVE_LDS : SLAB_STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* tl = lds + wave * MT_WAVE_LDS;      // this wave's tile
    float* rb = tl + MT_ROWS * MT_RS;          // residuals [draw][row]

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

    MTile t;
    load_mtile(t, X, ldx, y, row0_of(0), B, lane);
    for (int p = 0; p < n_iter; ++p) {
        // the tile to LDS, its registers take the next window's tile
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r) *reinterpret_cast<float4*>(tl + r * MT_RS + 4 * lane) = t.x[r];
        const float4 yv = t.yv;
        const int64_t rows_left = B - row0_of(p) - 4 * kq;     // rows 4 kq + reg < rows_left are real
        load_mtile(t, X, ldx, y, row0_of(p + 1), B, lane);
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
            const float r0 = glm_link<LINK>(d0[0] + d1[0], yv.x, rows_left > 0, ell);
            const float r1 = glm_link<LINK>(d0[1] + d1[1], yv.y, rows_left > 1, ell);
            const float r2 = glm_link<LINK>(d0[2] + d1[2], yv.z, rows_left > 2, ell);
            const float r3 = glm_link<LINK>(d0[3] + d1[3], yv.w, rows_left > 3, ell);
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
    float* ep = lds + wave * SLAB_STRIDE;
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
    __syncthreads();
    write_block_partial(lds, slab, tid);
}

// ---- float64 reduction of the slab: blr_slab_reduce_kernel's body, ell where that one writes Q -------------------
__global__ __launch_bounds__(RED_BLOCK) void glm_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks, int D,
                                                                    int S, int s_base, double* __restrict__ ell,
                                                                    double* __restrict__ G) {
    regress_slab_reduce(slab, n_blocks, D, S, s_base, ell, G);
}

// ---- the finish: slab reduce + ELBO + pathwise gradient + Adam + next draw, one launch ----------------------
//
// Grid = ceil(D / 8) column workgroups + 1 scalar workgroup (blr_fused_update_kernel's split).  A column
// workgroup owns 8 columns x 8 draws (one 256-byte run per slab row); the scalar workgroup owns ell, |w_s|^2, the
// entropy term and the ELBO.  lam = [m (D) | rho (D)] is double-buffered by the caller, so no workgroup reads what
// another one writes.
constexpr int FIN_BLOCK = 1024;
constexpr int FIN_WAVES = FIN_BLOCK / BSC_WAVE;

struct GlmArgs {
    const float* slab;       // block partials of the pass kernel, or nullptr
    int n_slab;
    const double* stats;     // [ell (S) | G (S*D)] when slab == nullptr
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;       // [S, D + 1] (bsc_blr_noise's layout; column D is not read)
    const float* W;
    const double* eps_next;  // nullptr: no next draw
    float* W_next;
    double* elbo;
    double* grad;
    int D, S;
    double scale, tau, c0;   // c0 = D/2 log(tau / 2 pi) + D/2 (1 + log 2 pi)
    bsc_adam adam;
};

__global__ __launch_bounds__(FIN_BLOCK) void glm_update_kernel(GlmArgs a) {
    __shared__ double red[FIN_WAVES][BSC_WAVE];
    __shared__ double sh[2 * MAX_S + 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, S = a.S;
    const int n_chunks = (D + 7) / 8;
    const int chunk = (int)blockIdx.x;   // == n_chunks: the scalar workgroup
    const double inv_S = 1.0 / (double)S;

    if (chunk < n_chunks) {
        // ---------------- column workgroup: columns d0 .. d0 + 7 ----------------
        const int d0 = 8 * chunk;
        const int dl = lane >> 3, sl = lane & 7;  // slab order within the run is [d][s]
        const int d = d0 + dl;
        double gm = 0.0, gr = 0.0;
        // every small operand of wave 0 is requested before the slab: one memory round trip for the workgroup
        double p_m = 0.0, p_rho = 0.0, p_m1 = 0.0, p_m2 = 0.0, p_r1 = 0.0, p_r2 = 0.0, e_next = 0.0;
        if (wave == 0) {
            if (sl == 0 && d < D) {
                p_m = a.lam_in[d]; p_rho = a.lam_in[D + d];
                p_m1 = a.m1[d]; p_m2 = a.m2[d];
                p_r1 = a.m1[D + d]; p_r2 = a.m2[D + d];
            }
            if (a.eps_next && sl < S && d < D) e_next = a.eps_next[(int64_t)sl * (D + 1) + d];
        }
        if (a.slab) {  // S <= 8: lane <-> (column dl, draw sl) of one 256-byte slab run
            const bool live = sl < S && d < D;
            double wv = 0.0, ev = 0.0;
            if (wave == 0 && live) {
                wv = (double)a.W[(int64_t)sl * D + d];
                ev = a.eps[(int64_t)sl * (D + 1) + d];
            }
            double s4[4];
            slab_run_sum<SLAB_STRIDE, FIN_WAVES>(a.slab, a.n_slab, 64 * chunk, wave, lane, s4, [] {});
            if (lane < 16) {
#pragma unroll
                for (int i = 0; i < 4; ++i) red[wave][4 * lane + i] = s4[i];
            }
            __syncthreads();
            if (wave != 0) return;
            double g = red[0][lane];
#pragma unroll
            for (int k = 1; k < FIN_WAVES; ++k) g += red[k][lane];
            if (live) {
                gm = a.scale * g - a.tau * wv;
                gr = gm * ev;
            }
        } else {
            if (wave != 0) return;
            for (int s = sl; s < S; s += 8) {
                if (d < D) {
                    const double wv = (double)a.W[(int64_t)s * D + d];
                    const double dw = a.scale * a.stats[S + (int64_t)s * D + d] - a.tau * wv;
                    gm += dw;
                    gr += dw * a.eps[(int64_t)s * (D + 1) + d];
                }
            }
        }
        // fold the 8 draw lanes (lane bits 0-2)
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            gm += __shfl_xor(gm, off);
            gr += __shfl_xor(gr, off);
        }
        double* new_m = sh;        // [8]
        double* new_sd = sh + 8;   // [8]
        if (sl == 0 && d < D) {
            const double g_m = gm * inv_S;
            const double g_r = gr * inv_S * exp(p_rho) + 1.0;
            a.grad[d] = g_m;
            a.grad[D + d] = g_r;
            const double nm = bsc_adam_ascent<true>(p_m, g_m, p_m1, p_m2, a.adam);
            a.m1[d] = p_m1; a.m2[d] = p_m2;
            const double nr = bsc_adam_ascent<true>(p_rho, g_r, p_r1, p_r2, a.adam);
            a.m1[D + d] = p_r1; a.m2[D + d] = p_r2;
            a.lam_out[d] = nm;
            a.lam_out[D + d] = nr;
            new_m[dl] = nm;
            new_sd[dl] = exp(nr);
        }
        wave_lds_sync();
        if (a.eps_next && d < D) {   // w = m + e^rho eps for this lane's (column, draws sl, sl + 8, ...)
            for (int s = sl; s < S; s += 8) {
                const double en = s == sl ? e_next : a.eps_next[(int64_t)s * (D + 1) + d];
                a.W_next[(int64_t)s * D + d] = (float)(new_m[dl] + new_sd[dl] * en);
            }
        }
        return;
    }

    // ---------------------------- scalar workgroup ----------------------------
    double* ells = sh;             // [S]
    double* wsq = sh + MAX_S;      // [S]
    double rho_part = 0.0;
    for (int d = tid; d < D; d += FIN_BLOCK) rho_part += a.lam_in[D + d];
    if (a.slab) {  // S <= 8: thread -> (draw tid & 7, slab-row group tid >> 3)
        double part = slab_column_sum<SLAB_STRIDE, 8>(a.slab + SLAB_G + (tid & 7), tid >> 3, FIN_BLOCK / 8, a.n_slab);
        part += __shfl_xor(part, 8);
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (lane < 8) red[wave][lane] = part;
    } else {
        for (int s = tid; s < S; s += FIN_BLOCK) ells[s] = a.stats[s];
    }
    // |w_s|^2: a wave per draw, fixed order
    for (int s = wave; s < S; s += FIN_WAVES) {
        double part = 0.0;
        for (int d = lane; d < D; d += BSC_WAVE) {
            const double wv = (double)a.W[(int64_t)s * D + d];
            part += wv * wv;
        }
        part = wave_allsum_f64(part);
        if (lane == 0) wsq[s] = part;
    }
    rho_part = wave_allsum_f64(rho_part);
    if (lane == 0) red[wave][32] = rho_part;  // column 32: clear of the ell staging columns
    __syncthreads();
    if (a.slab && tid < 8) {
        double t = 0.0;
        for (int k = 0; k < FIN_WAVES; ++k) t += red[k][tid];
        ells[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double sum_rho = 0.0;
        for (int k = 0; k < FIN_WAVES; ++k) sum_rho += red[k][32];
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += a.scale * ells[s] - 0.5 * a.tau * wsq[s];
        a.elbo[0] = fsum * inv_S + a.c0 + sum_rho;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------

// 16 = the MFMA kernel (needs the full 256-column layout and a 16-byte aligned y), else 8-row tiles.
int pass_rows(int D, const float* y) { return (D == GCOLS && (((uintptr_t)y) & 15) == 0) ? MT_ROWS : ROWS; }

// the link, then the envelope of every regression pass
int check_glm_args(const char* who, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                   const float* W, int32_t S, int max_s) {
    BSC_REQUIRE(link == BSC_GLM_LOGISTIC || link == BSC_GLM_POISSON,
                "%s: link=%d must be BSC_GLM_LOGISTIC (0) or BSC_GLM_POISSON (1)", who, link);
    BSC_REQUIRE(y || B <= 0, "%s: null pointer", who);
    return check_regress_args(who, X, ldx, B, D, W, S, max_s);
}

template <int LINK>
void launch_pass_link(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int D, const float* W,
                      int sg, PassGrid g, float* slab) {
    const dim3 grid(g.n_blocks), block(PASS_BLOCK);
    if (pass_rows(D, y) == MT_ROWS)
        hipLaunchKernelGGL((glm_pass_mfma_kernel<LINK>), grid, block, 0, ctx->stream, X, ldx, y, B, W, sg, slab,
                           g.n_iter);
    else if (D == GCOLS)
        hipLaunchKernelGGL((glm_pass_kernel<LINK, true>), grid, block, 0, ctx->stream, X, ldx, y, B, D, W, sg,
                           slab, g.n_iter);
    else
        hipLaunchKernelGGL((glm_pass_kernel<LINK, false>), grid, block, 0, ctx->stream, X, ldx, y, B, D, W, sg,
                           slab, g.n_iter);
}

void launch_pass(bsc_ctx* ctx, int link, const float* X, int64_t ldx, const float* y, int64_t B, int D, const float* W,
                 int sg, PassGrid g, float* slab) {
    bsc_prof_scope prof(ctx);  // times the pass kernel alone
    if (link == BSC_GLM_LOGISTIC) launch_pass_link<BSC_GLM_LOGISTIC>(ctx, X, ldx, y, B, D, W, sg, g, slab);
    else launch_pass_link<BSC_GLM_POISSON>(ctx, X, ldx, y, B, D, W, sg, g, slab);
}

int slab_for(bsc_ctx* ctx, PassGrid g, float** slab) {
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, (size_t)g.n_blocks * SLAB_STRIDE * sizeof(float), &ws);
    *slab = (float*)ws;
    return rc;
}

// The pass for S <= 8 draws, its block partials left in the workspace for the finish.
int pass_partial_impl(bsc_ctx* ctx, int link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                      const float* W, int32_t S) {
    const PassGrid g = pass_grid(ctx, B, pass_rows(D, y));
    float* slab = nullptr;
    const int rc = slab_for(ctx, g, &slab);
    if (rc != BSC_OK) return rc;
    launch_pass(ctx, link, X, ldx, y, B, (int)D, W, (int)S, g, slab);
    BSC_LAUNCH_CHECK();
    ctx->slab_rows = g.n_blocks;
    return BSC_OK;
}

int update_impl(bsc_ctx* ctx, const char* who, const double* stats, const double* lam_in, double* lam_out, double* m1,
                double* m2, const double* eps, const float* W, int32_t D, int32_t S, double scale, double tau, int64_t t,
                double lr, double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                double* eps_next, int32_t eps_next_ready, float* W_next, double* elbo, double* grad) {
    BSC_REQUIRE(lam_in && lam_out && m1 && m2 && eps && W && elbo && grad, "%s: null pointer", who);
    BSC_REQUIRE(lam_in != lam_out, "%s: lam_in and lam_out must differ", who);
    BSC_REQUIRE(D > 0 && S >= 1 && S <= MAX_S, "%s: D=%d S=%d (S<=%d)", who, D, S, MAX_S);
    BSC_REQUIRE(tau > 0.0, "%s: prior_precision=%g must be positive", who, tau);
    BSC_REQUIRE(scale > 0.0, "%s: scale=%g must be positive", who, scale);
    BSC_REQUIRE(t >= 1, "%s: the Adam step count starts at 1", who);
    BSC_REQUIRE((eps_next && W_next) || (!eps_next && !W_next), "%s: next-draw buffers must be both set or both null",
                who);
    BSC_REQUIRE(!eps_next || (eps_next != eps && W_next != W), "%s: next-draw buffers must not alias the current draws",
                who);
    GlmArgs a;
    a.stats = stats;
    a.slab = nullptr;
    a.n_slab = 0;
    if (!stats) {
        BSC_REQUIRE(ctx->slab_rows > 0 && ctx->workspace, "%s: stats is null and no pass partials are pending", who);
        BSC_REQUIRE(S <= SG && D <= GCOLS, "%s: slab input needs S<=8, D<=256", who);
        a.slab = (const float*)ctx->workspace;
        a.n_slab = ctx->slab_rows;
    }
    if (eps_next && !eps_next_ready) {   // the noise of next_step first (off the default path: drivers draw ahead)
        const int rc = bsc_blr_noise(ctx, D, S, seed, next_step, 1, eps_next);
        if (rc != BSC_OK) return rc;
    }
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.eps_next = eps_next; a.W_next = W_next;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.scale = scale; a.tau = tau;
    a.c0 = 0.5 * (double)D * (log(tau) - BSC_LOG_2PI) + 0.5 * (double)D * (1.0 + BSC_LOG_2PI);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
        hipLaunchKernelGGL(glm_update_kernel, dim3((D + 7) / 8 + 1), dim3(FIN_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    if (!stats) ctx->slab_rows = 0;   // the partials are consumed
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_glm_data_pass(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                      const float* W, int32_t S, double* ell, double* G) {
    BSC_CHECK_CTX(ctx);
    int rc = check_glm_args("bsc_glm_data_pass", link, X, ldx, y, B, D, W, S, MAX_S);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(ell && G, "bsc_glm_data_pass: null output");
    const PassGrid g = pass_grid(ctx, B, pass_rows(D, y));
    float* slab = nullptr;
    rc = slab_for(ctx, g, &slab);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    const dim3 rgrid((SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    for (int s0 = 0; s0 < S; s0 += SG) {   // eight draws per launch
        const int sg = S - s0 < SG ? S - s0 : SG;
        launch_pass(ctx, link, X, ldx, y, B, (int)D, W + (int64_t)s0 * D, sg, g, slab);
        BSC_LAUNCH_CHECK();
        hipLaunchKernelGGL(glm_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, slab, g.n_blocks, (int)D,
                           (int)S, s0, ell, G);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

int bsc_glm_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                   const double* eps, const float* W, int32_t D, int32_t S, double scale, double prior_precision,
                   int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                   double* eps_next, int32_t eps_next_ready, float* W_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return update_impl(ctx, "bsc_glm_update", stats, lam_in, lam_out, m1, m2, eps, W, D, S, scale, prior_precision, t, lr,
                       beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, elbo, grad);
}

int bsc_glm_pass_update(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                        const double* lam_in, double* lam_out, double* m1, double* m2, const double* eps, const float* W,
                        int32_t S, double scale, double prior_precision, int64_t t, double lr, double beta1, double beta2,
                        double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                        float* W_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    int rc = check_glm_args("bsc_glm_pass_update", link, X, ldx, y, B, D, W, S, SG);
    if (rc != BSC_OK) return rc;
    rc = pass_partial_impl(ctx, link, X, ldx, y, B, D, W, S);
    if (rc != BSC_OK) return rc;
    return update_impl(ctx, "bsc_glm_pass_update", nullptr, lam_in, lam_out, m1, m2, eps, W, D, S, scale, prior_precision,
                       t, lr, beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, elbo, grad);
}

}  // extern "C"
