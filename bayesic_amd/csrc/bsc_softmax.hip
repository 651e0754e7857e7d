// Reparameterised SVI for multi-class softmax regression: the data pass and the posterior predictive.
//
// ABSENT in the reference (README.md:51, 69-79 name the method; it has no inference code).  Labels y_n in {0 .. K-1},
// weights w in R^{K x D} under w ~ N(0, I / tau) on all K D entries (no reference class: the prior makes the posterior
// proper).  With l[n,s,k] = x_n . W[s,k,:] and lse[n,s] = logsumexp_k l[n,s,k] the data-sized work of one update is
//     ell[s]    = sum_n ( l[n,s,y_n] - lse[n,s] )
//     G[s,k,:]  = sum_n ( 1[y_n = k] - softmax_k(l[n,s,:]) ) x_n
// which is csrc/bsc_glm.hip's pass with K logits per (row, draw) instead of one.  The sixteen columns of the forward
// MFMA are (draw, class) pairs: one launch takes g = floor(16 / K) draws, column c = s_local K + k, columns >= g K zero.
//
// softmax_pass_kernel (one kernel for the whole envelope, D % 4 == 0 up to 256, 2 <= K <= 16): a wave owns 16-row
// tiles, prefetched through registers (non-temporal buffer loads: X is read once per launch; lane l holds columns
// 4 l .. 4 l + 3 of every row, columns >= D masked to zero) and parked row-major in the wave's LDS region.
//   forward   v_mfma_f32_16x16x4_f32 with the draws as the B operand: lane (c = lane % 16, kq = lane / 16) contracts
//             columns kq cw .. kq cw + cw - 1 (cw = 8 ceil(D / 32): the four lane groups share the D columns) and ends
//             with the logits of rows 4 kq .. 4 kq + 3 of column c, which go to LDS as lg[row][c].
//   softmax   lane (row = lane % 16, slot = lane / 16) owns the pairs (row, draw slot) and (row, draw slot + 4): the K
//             logits in registers, the maximum subtracted, ell accumulated in the lane, the residuals written back as
//             rb[c][row].  A row past the end of the batch reads as zeros through the buffer descriptor; its softmax
//             is not zero, so it is masked out of ell and of the residuals here.  A row whose label is outside [0, K)
//             is masked the same way: the label is only ever compared with class indices, never used as an address.
//   backward  the rank-1 updates G[c, :] += r[n, c] x[n, :] on v_mfma_f32_4x4x1_16B_f32, four column groups x four
//             column components (register i of accumulator (sb, q) = G[4 sb + i][4 lane + q]).
// Per-workgroup float32 partials [c][d] | ell[8] go to the context workspace and are summed in float64 in block
// order by softmax_slab_reduce_kernel: fixed partition, no float atomics, bitwise reproducible.
//
// softmax_predict_kernel: the forward half and the softmax only.  The tile stays in LDS while the kernel walks the
// draw groups (the draws of a group are re-read from the L2), so X is read once for every S; a lane keeps the running
// class probabilities and the running log-mean-exp of its (row, slot) pairs, the four slots of a row are folded by two
// butterflies, lanes 0 .. 15 store one row each.  lpd_sum: float64 lane sums -> wave -> block partial -> one
// fixed-order finish.
#include "bsc_regress.h"

namespace {

constexpr int NCOL = 16;                      // (draw, class) columns per launch: the MFMA's N
constexpr int MAX_K = 16;
constexpr int MAX_S = 64;
constexpr int MAX_G = 8;                      // draws per launch at K = 2
constexpr int T_ROWS = 16;                    // rows per tile
constexpr int T_RS = GCOLS + 4;               // LDS row stride of the tile (floats)
constexpr int LG_RS = NCOL + 1;               // logits lg[row][c]: odd stride, the K-loop of 64 lanes spreads over banks
constexpr int LG_FLOATS = T_ROWS * LG_RS;     // 272
constexpr int RB_RS = T_ROWS + 4;             // residuals rb[c][row]: 16-byte rows, draws land in different banks
constexpr int RB_FLOATS = NCOL * RB_RS;       // 320
constexpr int TILE_FLOATS = T_ROWS * T_RS;
constexpr int WAVE_LDS = TILE_FLOATS + LG_FLOATS + RB_FLOATS;
constexpr int SLAB_G = NCOL * GCOLS;          // slab[b][c * 256 + d], then ell at [SLAB_G + s_local]
constexpr int SLAB_STRIDE = SLAB_G + MAX_G;   // floats per block partial
constexpr int P_WAVE_LDS = TILE_FLOATS + LG_FLOATS;

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

struct Tile {
    float4 x[T_ROWS];
    int yv;        // y[row0 + lane % 16]: the row of this lane's softmax
};

// One tile = 16 rows from row0 on, through descriptors that cover exactly the rows [row0, B): later rows read zeros.
__device__ __forceinline__ void load_tile(Tile& t, const float* __restrict__ X, int64_t ldx,
                                          const int32_t* __restrict__ y, int64_t row0, int64_t B, int D, int lane) {
    auto xs = bsc_rows_rsrc(X, ldx, D, B, row0);
    auto ys = bsc_vec_rsrc(y, y ? B : 0, row0);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < T_ROWS; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, 2);   // non-temporal
        float4 f = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                               __uint_as_float(v[3]));
        if (4 * lane >= D) f = make_float4(0.f, 0.f, 0.f, 0.f);   // padding, or the next row's bytes
        t.x[r] = f;
    }
    t.yv = (int)__builtin_amdgcn_raw_buffer_load_b32(ys, 4 * (lane & 15), 0, 0);   // 4-byte loads: any alignment
}

__device__ __forceinline__ void park_tile(float* tl, const Tile& t, int lane) {
#pragma unroll
    for (int r = 0; r < T_ROWS; ++r) *reinterpret_cast<float4*>(tl + r * T_RS + 4 * lane) = t.x[r];
}

// Forward B operand of one draw group: Wg[c][kq cw + 4 j + e], zero for c >= ncols and columns >= D.
__device__ __forceinline__ void load_w(float (&wreg)[GCOLS / 4], const float* __restrict__ Wg, int D, int ncols, int cw,
                                       int i16, int kq) {
#pragma unroll
    for (int j = 0; j < GCOLS / 16; ++j) {
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const int col = kq * cw + 4 * j;
        if (4 * j < cw && col < D && i16 < ncols) w4 = *reinterpret_cast<const float4*>(Wg + (int64_t)i16 * D + col);
        wreg[4 * j + 0] = w4.x; wreg[4 * j + 1] = w4.y;
        wreg[4 * j + 2] = w4.z; wreg[4 * j + 3] = w4.w;
    }
}

// Logits of the parked tile for the sixteen columns of wreg, to lg[row][c] (two accumulators: no MFMA waits on its
// predecessor).  cw is a multiple of 8, so the unrolled steps leave in pairs.
__device__ __forceinline__ void forward_to_lds(const float* tl, float* lg, const float (&wreg)[GCOLS / 4], int cw,
                                               int i16, int kq) {
    mfma_f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
    const float* arow = tl + i16 * T_RS + kq * cw;
#pragma unroll
    for (int j = 0; j < GCOLS / 16; j += 2) {
        if (4 * j < cw) {
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
    }
    // register reg of lane (c = i16, kq) = logit(row 4 kq + reg, column c)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) lg[(4 * kq + reg) * LG_RS + i16] = d0[reg] + d1[reg];
}

// The K logits of one (row, draw) from lp[0 .. K-1] -> e[k] = exp(l_k - max), their sum, the maximum and l_y
// (0 when the label matches no class).  Finite for every finite logit: the largest exponent is 0.
__device__ __forceinline__ void softmax_terms(const float* lp, int K, int yv, float (&e)[MAX_K], float& mx, float& sum,
                                              float& ly) {
    mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        if (k < K) {
            e[k] = lp[k];
            mx = fmaxf(mx, e[k]);
        }
    }
    sum = 0.f;
    ly = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        if (k < K) {
            ly = yv == k ? e[k] : ly;
            e[k] = expf(e[k] - mx);
            sum += e[k];
        }
    }
}

// n_iter: tiles per wave (the same for every wave; tiles past the end read zeros).  sg draws, ncols = sg K columns.
__global__ __launch_bounds__(PASS_BLOCK, 2) void softmax_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const int32_t* __restrict__ y, int64_t B, int D, int K,
    const float* __restrict__ Wg, int sg, float* __restrict__ slab, int n_iter) {
    constexpr int LDS_FLOATS = PASS_WAVES * (WAVE_LDS > SLAB_STRIDE ? WAVE_LDS : SLAB_STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;     // forward: (column, k group); softmax: (row, draw slot)
    float* tl = lds + wave * WAVE_LDS;             // this wave's tile
    float* lg = tl + TILE_FLOATS;                  // logits [row][c]
    float* rb = lg + LG_FLOATS;                    // residuals [c][row]
    const int ncols = sg * K;
    const int cw = 8 * ((D + 31) / 32);

    float wreg[GCOLS / 4];
    load_w(wreg, Wg, D, ncols, cw, i16, kq);
    mfma_f32x4 acc[NCOL / 4][4];                   // [column group][column component]: register i = column 4 sb + i
#pragma unroll
    for (int sb = 0; sb < NCOL / 4; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[sb][q] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    float ell0 = 0.f, ell1 = 0.f;                  // draws kq and kq + 4, rows i16 of every tile
    for (int i = lane; i < RB_FLOATS; i += BSC_WAVE) rb[i] = 0.f;   // columns >= ncols stay zero for the backward

    // iteration p of every wave reads one contiguous window of gridDim.x * 4 tiles; p == n_iter: the empty tile
    const int64_t stride0 = (int64_t)gridDim.x * PASS_WAVES;
    const int64_t slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
    auto row0_of = [=](int p) { return p < n_iter ? ((int64_t)p * stride0 + slot) * T_ROWS : B; };

    Tile t;
    load_tile(t, X, ldx, y, row0_of(0), B, D, lane);
    for (int p = 0; p < n_iter; ++p) {
        park_tile(tl, t, lane);
        const int yv = t.yv;
        const bool real = row0_of(p) + i16 < B;
        load_tile(t, X, ldx, y, row0_of(p + 1), B, D, lane);
        wave_lds_sync();

        forward_to_lds(tl, lg, wreg, cw, i16, kq);
        wave_lds_sync();

        // softmax of (row i16, draws kq and kq + 4); a skipped row leaves zero residuals and nothing in ell
        const bool valid = real && (unsigned)yv < (unsigned)K;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int draw = kq + 4 * h;
            if (draw < sg) {
                float e[MAX_K], mx, sum, ly;
                softmax_terms(lg + i16 * LG_RS + draw * K, K, yv, e, mx, sum, ly);
                const float inv = valid ? 1.0f / sum : 0.f;
                const float lp = valid ? ly - (mx + logf(sum)) : 0.f;
                if (h == 0) ell0 += lp; else ell1 += lp;
                float* rp = rb + draw * K * RB_RS + i16;
#pragma unroll
                for (int k = 0; k < MAX_K; ++k)
                    if (k < K) rp[k * RB_RS] = ((valid && yv == k) ? 1.0f : 0.f) - e[k] * inv;
            }
        }
        wave_lds_sync();

        // backward on v_mfma_f32_4x4x1_16B_f32: per row up to four column groups x four column components
#pragma unroll
        for (int g = 0; g < T_ROWS / 4; ++g) {
            if (g) asm volatile("" ::: "memory");   // four rows of reads in flight
            float4 ra[NCOL / 4];
#pragma unroll
            for (int sb = 0; sb < NCOL / 4; ++sb)
                ra[sb] = *reinterpret_cast<const float4*>(rb + (4 * sb + (lane & 3)) * RB_RS + 4 * g);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float4 x4 = *reinterpret_cast<const float4*>(tl + (4 * g + rr) * T_RS + 4 * lane);
#pragma unroll
                for (int sb = 0; sb < NCOL / 4; ++sb) {
                    if (4 * sb < ncols) {
                        const float a = rr == 0 ? ra[sb].x : rr == 1 ? ra[sb].y : rr == 2 ? ra[sb].z : ra[sb].w;
                        acc[sb][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.x, acc[sb][0], 0, 0, 0);
                        acc[sb][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.y, acc[sb][1], 0, 0, 0);
                        acc[sb][2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.z, acc[sb][2], 0, 0, 0);
                        acc[sb][3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.w, acc[sb][3], 0, 0, 0);
                    }
                }
            }
        }
        wave_lds_sync();   // the next iteration overwrites the tile
    }

    __syncthreads();       // every wave is done with its private region
    float* ep = lds + wave * SLAB_STRIDE;
#pragma unroll
    for (int sb = 0; sb < NCOL / 4; ++sb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(ep + (4 * sb + i) * GCOLS + 4 * lane) =
                make_float4(acc[sb][0][i], acc[sb][1][i], acc[sb][2][i], acc[sb][3][i]);
    const float e0 = row16_allsum(ell0), e1 = row16_allsum(ell1);   // over the tile rows (lane bits 0 .. 3)
    if (i16 == 0) {
        ep[SLAB_G + kq] = e0;
        ep[SLAB_G + 4 + kq] = e1;
    }
    __syncthreads();
    // the block partial: fixed order over the waves
    float* out = slab + (int64_t)blockIdx.x * SLAB_STRIDE;
    for (int i = tid; i < SLAB_STRIDE; i += PASS_BLOCK) {
        float v = lds[i];
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) v += lds[k * SLAB_STRIDE + i];
        out[i] = v;
    }
}

// ---- float64 reduction of the slab: one output per lane, the 16 waves of a block split the slab rows and combine
//      through LDS in wave order ------------------------------------------------------------------------------------
__global__ __launch_bounds__(RED_BLOCK) void softmax_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                        int D, int K, int s0, int sg,
                                                                        double* __restrict__ ell,
                                                                        double* __restrict__ G) {
    __shared__ double part[RED_WAVES][BSC_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = blockIdx.x * BSC_WAVE + lane;
    double sum = 0.0;
    if (i < SLAB_STRIDE)
        for (int b = wave; b < n_blocks; b += RED_WAVES) sum += (double)slab[(int64_t)b * SLAB_STRIDE + i];
    part[wave][lane] = sum;
    __syncthreads();
    if (wave != 0 || i >= SLAB_STRIDE) return;
    double tot = part[0][lane];
#pragma unroll
    for (int k = 1; k < RED_WAVES; ++k) tot += part[k][lane];
    if (i < SLAB_G) {
        const int c = i / GCOLS, d = i % GCOLS;
        if (c < sg * K && d < D) G[((int64_t)s0 * K + c) * D + d] = tot;
    } else {
        const int s = i - SLAB_G;
        if (s < sg) ell[s0 + s] = tot;
    }
}

// ---- the posterior predictive -------------------------------------------------------------------------------------

struct PredictArgs {
    const float* X;
    int64_t ldx;
    const int32_t* y;        // may be null
    int64_t B;
    const float* W;
    float* prob;             // outputs, each may be null
    float* lpd;
    double* partial;         // [gridDim.x] block sums of lpd
    int D, K, S;
    int n_iter;              // tiles per wave
    int do_lp;               // y is set and lpd or lpd_sum is wanted
};

__global__ __launch_bounds__(PASS_BLOCK, 2) void softmax_predict_kernel(PredictArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[PASS_WAVES * P_WAVE_LDS];
    __shared__ double red[PASS_WAVES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* tl = lds + wave * P_WAVE_LDS;
    float* lg = tl + TILE_FLOATS;
    const int D = a.D, K = a.K, S = a.S;
    const int g = NCOL / K;                        // draws per group
    const int cw = 8 * ((D + 31) / 32);
    const int n_iter = a.n_iter;
    const int64_t B = a.B;
    const float inv_S = 1.0f / (float)S;
    const float log_S = logf((float)S);
    const bool one_group = S <= g;

    float wreg[GCOLS / 4];
    if (one_group) load_w(wreg, a.W, D, S * K, cw, i16, kq);

    const int64_t stride0 = (int64_t)gridDim.x * PASS_WAVES;
    const int64_t slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
    auto row0_of = [=](int p) { return p < n_iter ? ((int64_t)p * stride0 + slot) * T_ROWS : B; };
    double lsum = 0.0;

    Tile t;
    load_tile(t, a.X, a.ldx, a.y, row0_of(0), B, D, lane);
    for (int p = 0; p < n_iter; ++p) {
        park_tile(tl, t, lane);
        const int yv = t.yv;
        const int64_t row = row0_of(p) + i16;
        load_tile(t, a.X, a.ldx, a.y, row0_of(p + 1), B, D, lane);
        wave_lds_sync();

        float pk[MAX_K];                           // running sum over this lane's draws of softmax_k
#pragma unroll
        for (int k = 0; k < MAX_K; ++k) pk[k] = 0.f;
        float lmx = -INFINITY, lse = 0.f;          // running log-sum-exp of log p(y | draw): sum = lse * exp(lmx)
        for (int s0 = 0; s0 < S; s0 += g) {
            const int sg = S - s0 < g ? S - s0 : g;
            if (!one_group) load_w(wreg, a.W + (int64_t)s0 * K * D, D, sg * K, cw, i16, kq);
            forward_to_lds(tl, lg, wreg, cw, i16, kq);
            wave_lds_sync();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int draw = kq + 4 * h;
                if (draw < sg) {
                    float e[MAX_K], mx, sum, ly;
                    softmax_terms(lg + i16 * LG_RS + draw * K, K, yv, e, mx, sum, ly);
                    const float inv = 1.0f / sum;
#pragma unroll
                    for (int k = 0; k < MAX_K; ++k)
                        if (k < K) pk[k] = fmaf(e[k], inv, pk[k]);
                    if (a.do_lp) {
                        const float lp = ly - (mx + logf(sum));
                        const float nm = fmaxf(lmx, lp);
                        lse = lse * expf(lmx - nm) + expf(lp - nm);   // lmx = -inf: 0 * 0 + 1
                        lmx = nm;
                    }
                }
            }
            wave_lds_sync();   // the next group overwrites the logits
        }
        // the four slots of a row: class probabilities by two butterflies, the log-mean-exp about the row's maximum
#pragma unroll
        for (int k = 0; k < MAX_K; ++k)
            if (k < K) pk[k] = fold4_sum(pk[k]);
        float lpd = 0.f;
        if (a.do_lp) {
            float gm = fmaxf(lmx, __shfl_xor(lmx, 16));
            gm = fmaxf(gm, __shfl_xor(gm, 32));    // finite: slot 0 always holds a draw
            const float se = fold4_sum(lmx == -INFINITY ? 0.f : lse * expf(lmx - gm));
            lpd = gm + logf(se) - log_S;
        }
        if (kq == 0 && row < B) {                  // lanes 0 .. 15: one row each
            if (a.prob) {
#pragma unroll
                for (int k = 0; k < MAX_K; ++k)
                    if (k < K) a.prob[row * K + k] = pk[k] * inv_S;
            }
            if (a.do_lp) {
                const bool valid = (unsigned)yv < (unsigned)K;
                if (a.lpd) a.lpd[row] = valid ? lpd : 0.f;
                lsum += valid ? (double)lpd : 0.0;
            }
        }
    }

    if (a.partial) {   // fixed order: lanes (butterfly) -> waves -> block
        const double ws = wave_allsum_f64(lsum);
        if (lane == 0) red[wave] = ws;
        __syncthreads();
        if (tid == 0) {
            double tot = red[0];
#pragma unroll
            for (int k = 1; k < PASS_WAVES; ++k) tot += red[k];
            a.partial[blockIdx.x] = tot;
        }
    }
}

// lpd_sum = the block partials in block order
__global__ __launch_bounds__(BSC_WAVE) void softmax_predict_sum_kernel(const double* __restrict__ partial, int n,
                                                                       double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

// ---- host side ---------------------------------------------------------------------------------------------------

// the envelope of every regression pass, with 2 <= K <= 16 where it has always been checked
int check_softmax_args(const char* who, const float* X, int64_t ldx, int64_t B, int32_t D, int32_t K, const float* W,
                       int32_t S) {
    int rc = check_regress_batch(who, X, B, W);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(K >= 2 && K <= MAX_K, "%s: K=%d must be in [2,%d]", who, K, MAX_K);
    rc = check_regress_shape(who, X, ldx, D, W, S, MAX_S);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE((B + T_ROWS - 1) / T_ROWS < ((int64_t)1 << 40), "%s: B=%lld is too large", who, (long long)B);
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_softmax_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, int64_t B, int32_t D, int32_t K,
                          const float* W, int32_t S, double* ell, double* G) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_softmax_data_pass";
    int rc = check_softmax_args(who, X, ldx, B, D, K, W, S);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(y || B == 0, "%s: y is null", who);
    BSC_REQUIRE(ell && G, "%s: null output (ell, G)", who);
    const PassGrid g = pass_grid(ctx, B, T_ROWS);
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (size_t)g.n_blocks * SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // pass partials that were pending in the workspace are gone
    float* slab = (float*)ws;
    const int per = NCOL / K;   // draws per launch
    const dim3 rgrid((SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    for (int s0 = 0; s0 < S; s0 += per) {
        const int sg = S - s0 < per ? S - s0 : per;
        {
            bsc_prof_scope prof(ctx);  // times the pass kernel alone
            hipLaunchKernelGGL(softmax_pass_kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, B,
                               (int)D, (int)K, W + (int64_t)s0 * K * D, sg, slab, g.n_iter);
        }
        BSC_LAUNCH_CHECK();
        hipLaunchKernelGGL(softmax_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, slab, g.n_blocks, (int)D,
                           (int)K, s0, sg, ell, G);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

int bsc_softmax_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, int64_t B, int32_t D,
                             int32_t K, const float* W, int32_t S, float* prob, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_softmax_predict_pass";
    int rc = check_softmax_args(who, X, ldx, B, D, K, W, S);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(prob || lpd || lpd_sum, "%s: no output requested", who);
    BSC_REQUIRE(y || B == 0 || (!lpd && !lpd_sum), "%s: lpd and lpd_sum need y", who);
    if (B == 0) {
        if (lpd_sum) BSC_HIP(hipMemsetAsync(lpd_sum, 0, sizeof(double), ctx->stream));
        return BSC_OK;
    }
    const PassGrid g = pass_grid(ctx, B, T_ROWS);
    PredictArgs a;
    a.X = X; a.ldx = ldx; a.y = y; a.B = B; a.W = W;
    a.prob = prob; a.lpd = lpd; a.partial = nullptr;
    a.D = D; a.K = K; a.S = S;
    a.n_iter = g.n_iter;
    a.do_lp = (y && (lpd || lpd_sum)) ? 1 : 0;
    if (lpd_sum) {
        void* ws = nullptr;
        rc = bsc_workspace(ctx, (size_t)g.n_blocks * sizeof(double), &ws);
        if (rc != BSC_OK) return rc;
        ctx->slab_rows = 0;   // pass partials that were pending in the workspace are gone
        a.partial = (double*)ws;
    }
    {
        bsc_prof_scope prof(ctx);
        hipLaunchKernelGGL(softmax_predict_kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(softmax_predict_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream, a.partial, g.n_blocks,
                           lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // extern "C"
