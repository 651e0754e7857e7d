// Scaffolding shared by the regression SVI passes and their finishes: csrc/bsc_blr.hip, bsc_glm.hip, bsc_softmax.hip,
// bsc_predict.hip, the two full-covariance finishes (csrc/bsc_fullrank.h) and the two-launch mean-field finishes
// (csrc/bsc_meanfield.h).  The host side ends with what every finishing entry point checks and does alike
// (check_meanfield_update, next_draw_noise).  Header-only, internal linkage: every
// .hip is compiled on its own without relocatable device code, so each gets its own copy and the named kernels stay
// in their files.  What lives here has to give the same bits wherever it is used (the mean-field and full-covariance
// finishes are compared bit for bit, the slab reduction promises the same bytes run to run), hence one definition.
// One exception, spelled out at bsc_adam_ascent: glm_update_kernel alone asks for FUSED_MOMENTS, the two fused
// multiply-adds it has always been compiled with, so the GLM mean-field finish agrees with the other three finishes
// to the last bit or two of the moments (tests: rtol 1e-12), not bit for bit.  There are still two Adam arithmetics;
// they now sit in one function, and which kernel uses which is written down.
#pragma once

#include <cmath>

#include "bsc_common.h"

namespace {

constexpr int SG = 8;                         // draws per pass
constexpr int PASS_BLOCK = 256;
constexpr int PASS_WAVES = PASS_BLOCK / BSC_WAVE;
constexpr int GCOLS = 256;                    // column capacity of the lane layout
constexpr int REG_SLAB_G = SG * GCOLS;        // BLR / GLM slab[b][d*8 + s], then eight scalars (Q or ell) at [REG_SLAB_G + s]
constexpr int REG_SLAB_STRIDE = REG_SLAB_G + SG;   // floats per block partial

// ---- wave-level arithmetic --------------------------------------------------------------------------------------

__device__ __forceinline__ float swap_add32(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ float swap_add16(float a, float b) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    float v = a.x * b.x;
    v = fmaf(a.y, b.y, v);
    v = fmaf(a.z, b.z, v);
    return fmaf(a.w, b.w, v);
}

__device__ __forceinline__ void axpy4(float4& acc, float c, const float4& x) {
    acc.x = fmaf(c, x.x, acc.x);
    acc.y = fmaf(c, x.y, acc.y);
    acc.z = fmaf(c, x.z, acc.z);
    acc.w = fmaf(c, x.w, acc.w);
}

__device__ __forceinline__ float fold4_sum(float v) {   // over the four lanes that share lane % 16 (lane bits 4, 5)
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ float fold4_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

// ---- the VALU tile: ROWS rows, lane l holds columns 4l..4l+3 of every row ------------------------------------------

// Geometry of one wave's tile, for ROWS = 8 (2 waves/SIMD) or 4 (3 waves/SIMD).
// A lane writes its ROWS*8 partial dots as one LDS row of PSTR floats; PSTR = 4 mod 32
// keeps the 16-byte writes conflict-free, and the row blocks read by the four (eight)
// lane groups start a multiple of 32 (64) floats apart, so the 16-byte column reads are
// conflict-free as well.
template <int ROWS>
struct Geo {
    static constexpr int NVAL = ROWS * SG;        // values per lane: 64 or 32
    static constexpr int PSTR = NVAL + 4;         // 68 or 36 floats
    static constexpr int NGRP = NVAL / 4;         // lanes per value group set: 16 or 8
    static constexpr int NQ = BSC_WAVE / NGRP;    // row subsets: 4 or 8
    static constexpr int RPQ = BSC_WAVE / NQ;     // lane-rows per subset: 16 or 8
    static constexpr int WAVE_LDS = BSC_WAVE * PSTR + NVAL;  // + residual broadcast buffer
    static constexpr int OCC = ROWS == 8 ? 2 : 3;  // waves per SIMD (VGPR budget 256 / 168)
};

template <int ROWS>
struct RowTile {
    float4 x[ROWS];
    float yv;
};

// After the transposing reduction lane k holds value v(k) = row*8 + sample.
template <int ROWS>
__device__ __forceinline__ int lane_value(int lane) {
    return 4 * (lane & (Geo<ROWS>::NGRP - 1)) + 2 * ((lane >> 5) & 1) + ((lane >> 4) & 1);
}

// (The load of a tile stays with each pass: csrc/bsc_blr.hip builds its two buffer descriptors inline, csrc/bsc_glm.hip
// through bsc_rows_rsrc / bsc_vec_rsrc.  The two spellings mean the same and compile differently, and either pass
// kernel picks up another register allocation and schedule from the other's -- or from a shared load that is handed
// the descriptors -- so each keeps the few lines that give it the instruction stream it has been measured with.)

// ---- float64 reduction of a slab of per-workgroup float32 partials, fixed order ----------------------------------

// float64 sum of p[b * STRIDE] over slab rows b = first, first+step, ...
// Loads are issued in batches of BATCH before any add: the partials were written by
// another kernel, so every load is a MALL/HBM round trip (~0.4 us) and a
// load-add-load-add chain would serialise them.
template <int STRIDE, int BATCH>
__device__ __forceinline__ double slab_column_sum(const float* __restrict__ p, int first,
                                                  int step, int n_rows) {
    double sum = 0.0;
    for (int b0 = first; b0 < n_rows; b0 += step * BATCH) {
        float v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int b = b0 + j * step;
            v[j] = b < n_rows ? p[(int64_t)b * STRIDE] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) sum += (double)v[j];
    }
    return sum;
}

// Float64 sums of a 64-column run of the slab (columns col0 .. col0+63) over the rows
// wave + n_waves * k that this wave owns: 16-byte buffer loads covering four rows apiece
// (lane = (row group lane>>4, column chunk lane&15)); rows past n_slab read as zero through
// the descriptor.  On return lanes 0-15 hold, in s4[0..3], the sums of columns
// col0 + 4*lane .. +3.  `between` runs after the first batch of loads has been issued and
// before it is consumed (work that does not depend on the slab; `[] {}` for none).
// Kept deliberately compact: these finishing kernels start instruction-cache cold behind the
// 165-us data pass, and straight-line code is fetched at ~0.5 us per 64 bytes -- the 32
// guarded scalar loads this replaces (1.5 KB of code) cost 10 us before the first load had
// even been issued (cycle counters, round 1).
// JJ: loads in flight per lane and trip (8: the finish kernels' 16 waves cover 512 rows in one trip; 32: four waves do).
template <int STRIDE, int N_WAVES, int JJ = 8, typename F>
__device__ __forceinline__ void slab_run_sum(const float* __restrict__ slab, int n_slab, int col0,
                                             int wave, int lane, double (&s4)[4], F between) {
    const uint64_t slab_bytes = (uint64_t)n_slab * STRIDE * 4u;
    auto rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)slab, 0, slab_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)slab_bytes, 0x00020000);
    const int q4 = lane >> 4, c16 = lane & 15;
    const int voff = ((wave + N_WAVES * q4) * STRIDE + col0 + 4 * c16) * 4;
    constexpr int BATCH_BYTES = 4 * N_WAVES * STRIDE * 4;           // 4 * N_WAVES rows per load
    s4[0] = s4[1] = s4[2] = s4[3] = 0.0;
    for (int base = 0; base < n_slab; base += 4 * JJ * N_WAVES) {   // one trip up to 4 JJ N_WAVES partials
        float4 v8[JJ];
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
            auto v = __builtin_amdgcn_raw_buffer_load_b128(
                rs, voff, base * (STRIDE * 4) + jj * BATCH_BYTES, 0);
            v8[jj] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                                 __uint_as_float(v[3]));
        }
        if (base == 0) between();
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
            s4[0] += (double)v8[jj].x; s4[1] += (double)v8[jj].y;
            s4[2] += (double)v8[jj].z; s4[3] += (double)v8[jj].w;
        }
    }
    // fold the four row groups (lane bits 4, 5)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s4[i] += __shfl_xor(s4[i], 16);
        s4[i] += __shfl_xor(s4[i], 32);
    }
}

// Sum block partials of the [d * 8 + s | 8 scalars] slab in float64, fixed order: the body of blr_slab_reduce_kernel
// and glm_slab_reduce_kernel.  One output per lane; the 16 waves of a block split the slab rows, then combine through
// LDS in wave order.  `scalar` is Q (BLR) or ell (GLM).  STRIDE = REG_SLAB_G + 16 (csrc/bsc_glm_nb.hip): a second run
// of eight scalars behind the first goes to `scalar2`.
constexpr int RED_BLOCK = 1024;
constexpr int RED_WAVES = RED_BLOCK / BSC_WAVE;

template <int STRIDE = REG_SLAB_STRIDE>
__device__ __forceinline__ void regress_slab_reduce(const float* __restrict__ slab, int n_blocks, int D, int S,
                                                    int s_base, double* __restrict__ scalar, double* __restrict__ G,
                                                    double* __restrict__ scalar2 = nullptr) {
    static_assert(STRIDE == REG_SLAB_STRIDE || STRIDE == REG_SLAB_G + 2 * SG, "one or two runs of eight scalars");
    __shared__ double part[RED_WAVES][BSC_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = blockIdx.x * BSC_WAVE + lane;
    double s4[4];
    slab_run_sum<STRIDE, RED_WAVES>(slab, n_blocks, blockIdx.x * BSC_WAVE, wave, lane, s4, [] {});
    if (lane < 16) {   // (columns past the stride in the last workgroup are read but never written out)
#pragma unroll
        for (int k = 0; k < 4; ++k) part[wave][4 * lane + k] = s4[k];
    }
    __syncthreads();
    if (wave == 0 && i < STRIDE) {
        double tot = part[0][lane];
#pragma unroll
        for (int k = 1; k < RED_WAVES; ++k) tot += part[k][lane];
        if (i < REG_SLAB_G) {
            int s = i & 7, d = i >> 3;
            if (s_base + s < S && d < D) G[(int64_t)(s_base + s) * D + d] = tot;
        } else if (STRIDE == REG_SLAB_STRIDE || i < REG_SLAB_G + SG) {
            int s = i - REG_SLAB_G;
            if (s_base + s < S) scalar[s_base + s] = tot;
        } else {
            int s = i - REG_SLAB_G - SG;
            if (s_base + s < S) scalar2[s_base + s] = tot;
        }
    }
}

// out[0] = the per-workgroup float64 partials in block order, by one wave: lane k takes blocks k, k + 64, ..., then
// one butterfly.  The body of predict_sum_kernel and softmax_predict_sum_kernel.
__device__ __forceinline__ void block_partial_sum(const double* __restrict__ partial, int n, double* __restrict__ out) {
    double s = 0.0;
    for (int b = threadIdx.x; b < n; b += BSC_WAVE) s += partial[b];
    s = wave_allsum_f64(s);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- Adam ascent ------------------------------------------------------------------------------------------------

// The scalars of one Adam step; corr = 1 - beta^t, the bias corrections of step t >= 1.
struct bsc_adam {
    double lr, beta1, beta2, eps, corr1, corr2;
};

inline bsc_adam bsc_adam_make(double lr, double beta1, double beta2, double eps, int64_t t) {
    return bsc_adam{lr, beta1, beta2, eps, 1.0 - pow(beta1, (double)t), 1.0 - pow(beta2, (double)t)};
}

// One entry of lam, ascending; m1 and m2 are updated in place.  No contraction into FMAs, so that every finish that
// calls this does the same arithmetic, bit for bit.  FUSED_MOMENTS is glm_update_kernel's alone: that kernel was first
// built with the compiler's default contraction, which folded the two moment updates into one fused multiply-add
// each, and it keeps them so that its results do not move (they differ from the others' in the last bit).
template <bool FUSED_MOMENTS = false>
__device__ __forceinline__ double bsc_adam_ascent(double lam, double g, double& m1, double& m2, const bsc_adam& a) {
#pragma clang fp contract(off)
    const double na = FUSED_MOMENTS ? fma(a.beta1, m1, (1.0 - a.beta1) * g) : a.beta1 * m1 + (1.0 - a.beta1) * g;
    const double nb = FUSED_MOMENTS ? fma(a.beta2, m2, (1.0 - a.beta2) * g * g) : a.beta2 * m2 + (1.0 - a.beta2) * g * g;
    m1 = na;
    m2 = nb;
    const double mhat = na / a.corr1;
    const double vhat = nb / a.corr2;
    return lam + a.lr * mhat / (sqrt(vhat) + a.eps);
}

// ---- host side: the passes -----------------------------------------------------------------------------------------

// Grid and per-wave trip count: fill the resident wave slots, then balance so
// that every wave runs the same number of (almost all real) tiles.
struct PassGrid {
    int n_blocks;
    int n_iter;
};

inline PassGrid pass_grid(const bsc_ctx* ctx, int64_t B, int rows, int waves_per_simd = 2) {
    const int64_t n_tiles = (B + rows - 1) / rows;
    const int64_t max_waves = (int64_t)waves_per_simd * 4 * ctx->cu_count;
    PassGrid g;
    if (n_tiles <= 0) {
        g.n_blocks = 1;
        g.n_iter = 0;
        return g;
    }
    const int64_t n_iter = (n_tiles + max_waves - 1) / max_waves;
    const int64_t waves = (n_tiles + n_iter - 1) / n_iter;
    g.n_blocks = (int)((waves + PASS_WAVES - 1) / PASS_WAVES);
    g.n_iter = (int)n_iter;
    return g;
}

// The envelope every regression pass shares, each message naming the entry point and the quantity, in two halves
// so that a pass with a check of its own between them (softmax: K) keeps the order its refusals have always had.
// y is the caller's to check: its type and whether it may be null differ between the passes.
inline int check_regress_batch(const char* who, const float* X, int64_t B, const float* W) {
    BSC_REQUIRE(B >= 0, "%s: B=%lld", who, (long long)B);
    BSC_REQUIRE((X || B == 0) && W, "%s: null pointer", who);
    return BSC_OK;
}

inline int check_regress_shape(const char* who, const float* X, int64_t ldx, int32_t D, const float* W, int32_t S,
                               int max_s) {
    BSC_REQUIRE(D > 0 && D <= GCOLS && D % 4 == 0, "%s: D=%d must be a multiple of 4 in [4,%d]", who, D, GCOLS);
    BSC_REQUIRE(S >= 1 && S <= max_s, "%s: S=%d must be in [1,%d]", who, S, max_s);
    BSC_REQUIRE(ldx >= D && ldx % 4 == 0 && ldx < ((int64_t)1 << 26),
                "%s: ldx=%lld must be >= D, %% 4 == 0 and < 2^26", who, (long long)ldx);
    BSC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: X and W must be 16-byte aligned", who);
    return BSC_OK;
}

inline int check_regress_args(const char* who, const float* X, int64_t ldx, int64_t B, int32_t D, const float* W,
                              int32_t S, int max_s) {
    const int rc = check_regress_batch(who, X, B, W);
    return rc != BSC_OK ? rc : check_regress_shape(who, X, ldx, D, W, S, max_s);
}

// ---- host side: what the finishing entry points check and do alike ------------------------------------------------

// The checks every mean-field finish makes of its state and its scalars, in the order they have always been made;
// `pointers_set`: the caller's own list.  has_gamma: the model has a Gamma(a0, b0) prior on a scalar latent.  A check
// of the model's own (stats, J) stays with the caller.
inline int check_meanfield_update(const char* who, bool pointers_set, const double* lam_in, const double* lam_out,
                                  int32_t D, int32_t S, int max_s, double prior_precision, bool has_gamma, double a0,
                                  double b0, double scale, int64_t t) {
    BSC_REQUIRE(pointers_set, "%s: null pointer", who);
    BSC_REQUIRE(lam_in != lam_out, "%s: lam_in and lam_out must differ", who);
    BSC_REQUIRE(D > 0 && S >= 1 && S <= max_s, "%s: D=%d S=%d (S<=%d)", who, D, S, max_s);
    BSC_REQUIRE(prior_precision > 0.0, "%s: prior_precision=%g must be positive", who, prior_precision);
    BSC_REQUIRE(!has_gamma || (a0 > 0.0 && b0 > 0.0), "%s: a0=%g b0=%g must be positive", who, a0, b0);
    BSC_REQUIRE(scale > 0.0, "%s: scale=%g must be positive", who, scale);
    BSC_REQUIRE(t >= 1, "%s: the Adam step count starts at 1", who);
    return BSC_OK;
}

// The next-draw buffers (all set or all null, none of them its current twin; has_extra: the model has a latent besides
// W with buffers of its own -- xi, Bz, logphi), then the next step's noise in bsc_blr_noise's layout, `noise_dim`
// stream-0 columns, unless the caller has drawn it.
inline int next_draw_noise(bsc_ctx* ctx, const char* who, bool has_extra, const double* eps, const float* W,
                           const void* extra, double* eps_next, float* W_next, const void* extra_next,
                           int32_t noise_dim, int32_t S, uint64_t seed, uint32_t next_step, int32_t eps_next_ready) {
    const char* how_many = has_extra ? "all" : "both";
    BSC_REQUIRE((eps_next && W_next && (extra_next || !has_extra)) || (!eps_next && !W_next && !extra_next),
                "%s: next-draw buffers must be %s set or %s null", who, how_many, how_many);
    BSC_REQUIRE(!eps_next || (eps_next != eps && W_next != W && (!has_extra || extra_next != extra)),
                "%s: next-draw buffers must not alias the current draws", who);
    if (eps_next && !eps_next_ready) return bsc_blr_noise(ctx, noise_dim, S, seed, next_step, 1, eps_next);
    return BSC_OK;
}

}  // namespace
