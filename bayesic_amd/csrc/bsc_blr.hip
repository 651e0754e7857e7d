// Bayesian-linear-regression reparameterised ELBO path (BASELINE config 2).
//
// ABSENT in the reference: spec is README.md:51 (reparameterisation trick,
// refs [10][11][12]) and README.md:69-79 (mini-batch SVI), with the
// log-likelihood split of bayesic/distribution/base.py:47-69.
//
// blr_pass_kernel is the HBM-bound hot kernel: ONE read of X[B,D] and y[B]
// produces, for S<=8 Monte-Carlo weight draws at once,
//     Q[s]   = sum_n (y_n - x_n.w_s)^2
//     G[s,:] = sum_n (y_n - x_n.w_s) x_n
// Layout: a wave owns 8-row tiles; lane l holds columns 4l..4l+3 of every row
// (one 16-byte load per row per lane = 1 KiB coalesced per wave instruction at
// D=256).  The 64 per-lane partial dot products (8 rows x 8 samples) are
// transposed and summed through a wave-private LDS region (no workgroup
// barrier), the residuals are broadcast back through LDS, and the backward
// rank-1 updates accumulate into per-lane registers acc[s][4] that live for the
// whole kernel.  Measured VALU issue costs on gfx950 (profiles/
// r01_ubench_valu_issue_rates.txt: v_permlane*_swap 2.9x, DPP 1.5x, SGPR-operand
// FMA 1.55x a plain FMA) are why the cross-lane work rides the LDS pipe and
// every FMA is all-VGPR.  Block partials go to a slab; they are summed in
// float64 in a fixed order (bitwise reproducible, no float atomics).
#include "bsc_regress.h"

namespace {

constexpr int SLAB_G = REG_SLAB_G;            // slab[b][d*8 + s], then Q at [SLAB_G + s]
constexpr int SLAB_STRIDE = REG_SLAB_STRIDE;  // floats per block partial

// ---- block epilogue of the eight-draw passes: the four waves' partials summed in wave order, one slab row out -------
//
// In slab order [d * 8 + s] a lane's 32 accumulators (columns 4 lane .. 4 lane + 3, eight draws) are 128 contiguous
// bytes of the row: its 16-byte chunk j = 2 q + sb is column 4 lane + q, draws 4 sb .. 4 sb + 3, chunk 8 lane + j of the
// row.  So the transposition happens in registers while WRITING: each wave puts its chunks into its [SLAB_STRIDE] LDS
// region, and the sum over the waves reads whole chunks, consecutive threads consecutive chunks, and stores 16 bytes.
// Chunk c sits at chunk position slab_chunk_pos(c) -- its index within the lane's eight XORed with lane % 8 -- which
// keeps both sides conflict-free: the eight contiguous lanes of a ds_write_b128 group then cover eight different 16-byte
// slots of the 128-byte bank row, and the XOR maps aligned runs of four chunks onto aligned runs of four, so the
// sixteen lanes of a ds_read_b128 group still cover sixteen different slots of the 256-byte one.
__device__ __forceinline__ int slab_chunk_pos(int c) { return (c & ~7) | ((c & 7) ^ ((c >> 3) & 7)); }

template <typename V>
__device__ __forceinline__ void slab_chunk_put(float* __restrict__ ep, int lane, int j, const V& v) {
    static_assert(sizeof(V) == 16, "one 16-byte chunk");
    *reinterpret_cast<V*>(ep + 4 * slab_chunk_pos(8 * lane + j)) = v;
}

// `lds`: PASS_WAVES regions of SLAB_STRIDE floats (chunks as above, then the eight scalars); out: the slab row.
__device__ __forceinline__ void slab_row_out(const float* __restrict__ lds, float* __restrict__ out, int tid) {
    for (int c = tid; c < SLAB_G / 4; c += PASS_BLOCK) {
        const int p = 4 * slab_chunk_pos(c);
        float4 v = *reinterpret_cast<const float4*>(lds + p);
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) {
            const float4 u = *reinterpret_cast<const float4*>(lds + k * SLAB_STRIDE + p);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        *reinterpret_cast<float4*>(out + 4 * c) = v;
    }
    if (tid < SG) {
        float v = lds[SLAB_G + tid];
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) v += lds[k * SLAB_STRIDE + SLAB_G + tid];
        out[SLAB_G + tid] = v;
    }
}

// One tile = ROWS rows starting at row0, through buffer loads: the descriptor
// (SGPRs) covers exactly the rows [row0, B), so rows past the end -- and whole
// tiles past the end -- read as zeros without touching memory.  No ragged-tail
// code path and a trip count that is the same for every wave.  Everything but
// the 16*lane byte offset is wave-uniform.
template <int ROWS, bool FULL, bool NT>
__device__ __forceinline__ void load_tile(RowTile<ROWS>& t, const float* __restrict__ X,
                                          int64_t ldx, const float* __restrict__ y,
                                          int64_t row0, int64_t B, int D, int lane) {
    const int64_t rem = B - row0;  // rows left; <= 0 for a tile past the end
    uint64_t xbytes = 0, ybytes = 0;
    if (rem > 0) {
        xbytes = ((uint64_t)(rem - 1) * (uint64_t)ldx + (uint64_t)D) * 4u;
        ybytes = (uint64_t)rem * 4u;
    }
    const unsigned xrec = xbytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)xbytes;
    const unsigned yrec = ybytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)ybytes;
    const int64_t safe0 = rem > 0 ? row0 : 0;  // keep the base pointer inside the allocation
    auto xs = __builtin_amdgcn_make_buffer_rsrc((void*)(X + safe0 * ldx), 0, xrec, 0x00020000);
    auto ys = __builtin_amdgcn_make_buffer_rsrc((void*)(y + safe0), 0, yrec, 0x00020000);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        // NT: non-temporal (aux = 2) -- X is read exactly once per pass
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, NT ? 2 : 0);
        float4 f = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]),
                               __uint_as_float(v[2]), __uint_as_float(v[3]));
        if (!FULL && 4 * lane >= D) f = make_float4(0.f, 0.f, 0.f, 0.f);  // next row's bytes
        t.x[r] = f;
    }
    t.yv = __uint_as_float(
        __builtin_amdgcn_raw_buffer_load_b32(ys, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
}

// Forward + backward for one tile; `wl` is this wave's LDS region.
template <int ROWS>
__device__ __forceinline__ void compute_tile(const RowTile<ROWS>& t, const float4 (&w)[SG],
                                             float4 (&acc)[SG], float& qacc, float* wl,
                                             int lane) {
    using G = Geo<ROWS>;
    // 1. per-lane partial dots, row by row, into this lane's row of the buffer
    float* mine = wl + lane * G::PSTR;
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
    // 2. lane k sums values 4g..4g+3 (g = k % NGRP) over the lane-rows q*RPQ .. q*RPQ+RPQ-1
    const int g = lane & (G::NGRP - 1), q = lane / G::NGRP;
    const float* col = wl + q * G::RPQ * G::PSTR + 4 * g;
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int RB = ROWS == 8 ? 8 : 4;  // reads in flight before the first add
#pragma unroll
    for (int part = 0; part < G::RPQ / RB; ++part) {
        float4 v[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i)
            v[i] = *reinterpret_cast<const float4*>(col + (RB * part + i) * G::PSTR);
#pragma unroll
        for (int h = RB / 2; h >= 1; h >>= 1) {
#pragma unroll
            for (int i = 0; i < h; ++i) {
                v[i].x += v[i + h].x; v[i].y += v[i + h].y;
                v[i].z += v[i + h].z; v[i].w += v[i + h].w;
            }
        }
        s4.x += v[0].x; s4.y += v[0].y; s4.z += v[0].z; s4.w += v[0].w;
    }
    // 3. fold the row subsets (lane bits 4,5; and bit 3 when ROWS == 4): lane k ends
    //    with value lane_value(k)
    float t0 = swap_add32(s4.x, s4.z);
    float t1 = swap_add32(s4.y, s4.w);
    float dot = swap_add16(t0, t1);
    if (ROWS == 4) dot += dpp_f32<DPP_ROW_ROR8>(dot);  // lanes k and k^8 hold the same value
    float resid = t.yv - dot;
    qacc = fmaf(resid, resid, qacc);
    float* rb = wl + BSC_WAVE * G::PSTR;
    rb[lane_value<ROWS>(lane)] = resid;
    wave_lds_sync();
    // 4. backward: acc[s] += resid(r,s) * x[r]; residuals arrive by LDS broadcast
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        // keep at most four rows of broadcast reads in flight (register budget)
        if (r == 4) asm volatile("" ::: "memory");
        float4 c0 = *reinterpret_cast<const float4*>(rb + r * SG);
        float4 c1 = *reinterpret_cast<const float4*>(rb + r * SG + 4);
        axpy4(acc[0], c0.x, t.x[r]); axpy4(acc[1], c0.y, t.x[r]);
        axpy4(acc[2], c0.z, t.x[r]); axpy4(acc[3], c0.w, t.x[r]);
        axpy4(acc[4], c1.x, t.x[r]); axpy4(acc[5], c1.y, t.x[r]);
        axpy4(acc[6], c1.z, t.x[r]); axpy4(acc[7], c1.w, t.x[r]);
    }
}

// FULL: D == 256, every lane owns four live columns.  ROWS: tile height.
// n_iter: tiles per wave (same for every wave; tiles past the end read zeros).
template <bool FULL, int ROWS, bool NT>
__global__ __launch_bounds__(PASS_BLOCK, Geo<ROWS>::OCC) void blr_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B, int D,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter) {
    using G = Geo<ROWS>;
    // one array: wave-private regions during the loop, [wave][SLAB_STRIDE] in the epilogue
    constexpr int LDS_FLOATS = PASS_WAVES * (G::WAVE_LDS > SLAB_STRIDE ? G::WAVE_LDS : SLAB_STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // wave-uniform by construction; telling the compiler keeps tile indices and
    // buffer descriptors in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wl = lds + wave * G::WAVE_LDS;

    float4 w[SG], acc[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        w[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * lane < D && s < S)
            w[s] = *reinterpret_cast<const float4*>(W + (int64_t)s * D + 4 * lane);
        acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float qacc = 0.f;

    // This wave owns tiles first, first+stride, ... (n_iter of them).  Every
    // prefetch is unconditional -- a conditional one makes the compiler wait with
    // vmcnt(0), i.e. no prefetch at all -- and out-of-range tiles cost no traffic.
    const int64_t stride = (int64_t)gridDim.x * PASS_WAVES;
    int64_t tile = (int64_t)blockIdx.x * PASS_WAVES + wave;
    RowTile<ROWS> ta, tb;
    load_tile<ROWS, FULL, NT>(ta, X, ldx, y, tile * ROWS, B, D, lane);
    for (int k = 0; k + 1 < n_iter; k += 2) {
        load_tile<ROWS, FULL, NT>(tb, X, ldx, y, (tile + stride) * ROWS, B, D, lane);
        compute_tile<ROWS>(ta, w, acc, qacc, wl, lane);
        load_tile<ROWS, FULL, NT>(ta, X, ldx, y, (tile + 2 * stride) * ROWS, B, D, lane);
        compute_tile<ROWS>(tb, w, acc, qacc, wl, lane);
        tile += 2 * stride;
    }
    if (n_iter & 1) compute_tile<ROWS>(ta, w, acc, qacc, wl, lane);

    // block reduction through LDS, fixed order over waves
    __syncthreads();  // every wave is done with its private region
    float* ep = lds + wave * SLAB_STRIDE;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        const float4 &a0 = acc[4 * sb], &a1 = acc[4 * sb + 1], &a2 = acc[4 * sb + 2], &a3 = acc[4 * sb + 3];
        slab_chunk_put(ep, lane, 0 + sb, make_float4(a0.x, a1.x, a2.x, a3.x));
        slab_chunk_put(ep, lane, 2 + sb, make_float4(a0.y, a1.y, a2.y, a3.y));
        slab_chunk_put(ep, lane, 4 + sb, make_float4(a0.z, a1.z, a2.z, a3.z));
        slab_chunk_put(ep, lane, 6 + sb, make_float4(a0.w, a1.w, a2.w, a3.w));
    }
    // qacc of lane k belongs to sample lane_value(k)&7; fold the tile rows (lane bits 1..)
    // -- with ROWS == 4 lanes k and k^8 carry the same residuals, hence the 0.5
    float qv = qacc;
    qv += __shfl_xor(qv, 2);
    qv += __shfl_xor(qv, 4);
    qv += __shfl_xor(qv, 8);
    if (ROWS == 4) qv *= 0.5f;
    if ((lane & 14) == 0) ep[SLAB_G + (lane_value<ROWS>(lane) & 7)] = qv;
    __syncthreads();
    // slab order is [d][s] so that a finisher reads 8 columns x 8 samples as one 256-B run
    slab_row_out(lds, slab + (int64_t)blockIdx.x * SLAB_STRIDE, tid);
}

// ---- 16-row tiles for the kernels that contract on the MFMA pipe (D == 256) -----------------
//
// The kernel above keeps ~83 % of the VALU issue slots busy behind the HBM stream,
// so it slows down on boxes whose sustained shader clock is lower (measured: pure-read
// ceiling equal or higher, pass 10-20 % slower).  fp32 MFMA has the same peak as fp32
// VALU on this part, but it is a SEPARATE pipe: the kernels below put both contractions
// there.  A wave owns 16-row tiles, held row-major in the wave's LDS region (stride 260
// floats).
constexpr int MT_ROWS = 16;
constexpr int MT_RS = GCOLS + 4;                         // LDS row stride (floats)
constexpr int MT_WAVE_LDS = MT_ROWS * MT_RS + MT_ROWS * SG;   // tile + residual buffer

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

struct MTile {
    float4 x[MT_ROWS];
    float4 yv;     // y[row0 + 4 kq .. + 3]: the rows of this lane's MFMA result registers
};

template <int AUX>
__device__ __forceinline__ void load_mtile_policy(MTile& t, const float* __restrict__ X, int64_t ldx,
                                                  const float* __restrict__ y, int64_t row0, int64_t B,
                                                  int lane) {
    const int64_t rem = row0 < 0 ? 0 : B - row0;   // a window before row 0 is as empty as one past B
    uint64_t xbytes = 0, ybytes = 0;
    if (rem > 0) {
        xbytes = ((uint64_t)(rem - 1) * (uint64_t)ldx + (uint64_t)GCOLS) * 4u;
        ybytes = (uint64_t)rem * 4u;
    }
    const unsigned xrec = xbytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)xbytes;
    const unsigned yrec = ybytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)ybytes;
    const int64_t safe0 = rem > 0 ? row0 : 0;
    auto xs = __builtin_amdgcn_make_buffer_rsrc((void*)(X + safe0 * ldx), 0, xrec, 0x00020000);
    auto ys = __builtin_amdgcn_make_buffer_rsrc((void*)(y + safe0), 0, yrec, 0x00020000);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < MT_ROWS; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, AUX);
        t.x[r] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                             __uint_as_float(v[3]));
    }
    auto v = __builtin_amdgcn_raw_buffer_load_b128(ys, 16 * (lane >> 4), 0, 0);
    t.yv = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                       __uint_as_float(v[3]));
}

// The tile by LDS-DMA: buffer_load ... lds writes a row's 1 KiB straight into the wave's LDS tile: no 64 staging
// registers, no sixteen ds_write_b128 a tile, and on this part a pure read by LDS-DMA reaches 6.9 TB/s where loads into
// registers reach 6.4 (bsc_hbm_read_probe).  No LDS read of the tile may follow a DMA in flight: the compiler answers
// such a read with vmcnt(0) (q_tile_step orders its reads accordingly).
template <int AUX>
__device__ __forceinline__ void dma_mtile(float* __restrict__ tl, const float* __restrict__ X, int64_t ldx,
                                          const float* __restrict__ y, int64_t row0, int64_t B, int lane, float4& yv) {
    const int64_t rem = row0 < 0 ? 0 : B - row0;
    uint64_t xbytes = 0, ybytes = 0;
    if (rem > 0) {
        xbytes = ((uint64_t)(rem - 1) * (uint64_t)ldx + (uint64_t)GCOLS) * 4u;
        ybytes = (uint64_t)rem * 4u;
    }
    const unsigned xrec = xbytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)xbytes;
    const unsigned yrec = ybytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)ybytes;
    const int64_t safe0 = rem > 0 ? row0 : 0;
    auto xs = __builtin_amdgcn_make_buffer_rsrc((void*)(X + safe0 * ldx), 0, xrec, 0x00020000);
    auto ys = __builtin_amdgcn_make_buffer_rsrc((void*)(y + safe0), 0, yrec, 0x00020000);
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < MT_ROWS; ++r)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xs, (bsc_lds_ptr)(tl + r * MT_RS), 16, 16 * lane, r * row_bytes, 0, AUX);
    auto v = __builtin_amdgcn_raw_buffer_load_b128(ys, 16 * (lane >> 4), 0, 0);
    yv = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// ---- round 4: BOTH contractions on v_mfma_f32_4x4x1_16B_f32, the tile by LDS-DMA (D == 256, S <= 8) -----------------
//
// The counters of round 3's pass (forward on v_mfma_f32_16x16x4, backward on packed VALU FMAs, the tile by LDS-DMA;
// profiles/r03_pmc_blr_pass_dma.txt) say what held it at 0.80 of the peak: a
// 16-row tile costs a SIMD 64 v_mfma_f32_16x16x4 of 32 cycles (half of each idle: eight draws in sixteen columns) plus
// ~310 vector instructions at ~4.6 matrix-pipe cycles apiece (fp32 MFMA and VALU do not overlap on a SIMD:
// profiles/r01_ubench_mfma_valu_mix.txt) -- ~3 500 issue cycles a tile, ~0.75 of the time HBM takes to deliver it.
// v_mfma_f32_4x4x1 is sixteen independent 4 x 4 outer products (K = 1) in 8 cycles and has no idle half:
//
//   forward   block b = lane / 4 = (k8 = lane >> 3, sb = (lane >> 2) & 1) contracts the 32 columns
//             {128 h + 16 k8 + c : h < 2, c < 16} for the draws 4 sb .. 4 sb + 3: A = x[4 g + lane % 4][col] (the
//             rows of row group g, read from the LDS tile: eight ds_read_b128 a group, conflict-free because the four
//             k8 of a ds_read_b128 lane group start 16 floats apart), B = w[4 sb + lane % 4][col] (32 registers, loaded
//             once), and register i of accumulator g is the partial dot product (row 4 g + i, draw lane % 8) over
//             the lane's columns.  The eight column blocks are folded by two halving swaps (v_permlane32_swap,
//             v_permlane16_swap: each also halves the values a lane carries, 16 -> 8 -> 4) and one DPP rotation:
//             28 vector instructions a tile, after which lane (kq = lane >> 4, draw = lane % 8) holds the dot
//             products of rows 4 kq .. 4 kq + 3 -- the rows whose y it loaded.  128 MFMAs of 8 cycles.
//   backward  as blr_pass_mx_kernel: A = r[n][4 sb + lane % 4] (LDS broadcast), B = x[n][4 lane + q], register i of
//             accumulator (sb, q) is G[4 sb + i][4 lane + q].  128 MFMAs of 8 cycles.
//
// ~2 050 matrix-pipe cycles and ~45 vector instructions a tile.  The feed (dma_mtile): one 16-row buffer
// per wave; every operand of the backward (sixteen rows, the residuals) goes to registers before the next tile's
// sixteen DMAs are issued, so those have the backward and the other wave's turn to land.
constexpr int QW = 32;   // forward B operand: registers per lane

// DBG (profiling only, WRONG results; BSC_BLR_Q_DBG + BSC_PROFILING_BUILDS): 1 = no arithmetic at all (the feed's own
// ceiling: DMAs, waits, LDS reads), 2 = forward only, 3 = backward only
// `next_row0()` is called once, right before the next tile's DMAs are issued: evaluated earlier, its result would be
// live across the forward (4 VGPRs more).
template <int AUX, int DBG, int PRIO, typename NextRow>
__device__ __forceinline__ void q_tile_step(float4& yv_cur, float* __restrict__ tl, float* __restrict__ rb,
                                            const float (&wreg)[QW], mfma_f32x4 (&acc)[2][4], float& qacc,
                                            const float* __restrict__ X, int64_t ldx, const float* __restrict__ y,
                                            NextRow next_row0, int64_t B, int lane) {
    const int kq = lane >> 4;
    // the tile's DMAs (issued a step ago) and its y have landed
    __builtin_amdgcn_s_waitcnt(bsc_vmcnt_only(0));
    asm volatile("" ::: "memory");
    // PRIO 1: the stretch from "my tile has landed" to "my next tile's DMAs are out" runs at raised priority -- it is
    // the latency chain that sets how fast a wave can draw on HBM; the backward, which only has to finish before
    // the next tile lands, yields to the partner wave's forward.  (PRIO 2: the other way round, for the A/B.)
    if (PRIO == 1) __builtin_amdgcn_s_setprio(1);
    if (PRIO == 2) __builtin_amdgcn_s_setprio(0);
    const float4 yv = yv_cur;
    if (DBG == 0 || DBG == 2) {
        mfma_f32x4 d[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) d[g] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
        const float* abase = tl + (lane & 3) * MT_RS + 16 * (lane >> 3);
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
            float4 a[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                a[g] = *reinterpret_cast<const float4*>(abase + 4 * g * MT_RS + 128 * (c8 >> 2) + 4 * (c8 & 3));
#pragma unroll
            for (int g = 0; g < 4; ++g) d[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[g].x, wreg[4 * c8 + 0], d[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) d[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[g].y, wreg[4 * c8 + 1], d[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) d[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[g].z, wreg[4 * c8 + 2], d[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) d[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[g].w, wreg[4 * c8 + 3], d[g], 0, 0, 0);
        }
        // fold the eight column blocks (lane bits 5, 4, 3); lanes l and l ^ 8 end with the same four values
        float u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t0 = swap_add32(d[0][i], d[2][i]);    // lanes 0..31: row group 0, lanes 32..63: row group 2
            const float t1 = swap_add32(d[1][i], d[3][i]);    //              row group 1               row group 3
            float v = swap_add16(t0, t1);                     // DPP rows 0, 2 keep t0, rows 1, 3 t1: row group kq
            v += dpp_f32<DPP_ROW_ROR8>(v);
            u[i] = v;
        }
        const float r0 = yv.x - u[0], r1 = yv.y - u[1], r2 = yv.z - u[2], r3 = yv.w - u[3];
        qacc = fmaf(r0, r0, qacc); qacc = fmaf(r1, r1, qacc);
        qacc = fmaf(r2, r2, qacc); qacc = fmaf(r3, r3, qacc);
        // rb[draw][row]; both lanes of a pair (l, l ^ 8) store the same sixteen bytes
        *reinterpret_cast<float4*>(rb + (lane & 7) * MT_ROWS + 4 * kq) = make_float4(r0, r1, r2, r3);
    }
    wave_lds_sync();
    // every operand of the backward into registers, then the buffer belongs to the next tile
    float4 x4[MT_ROWS];
#pragma unroll
    for (int r = 0; r < MT_ROWS; ++r) x4[r] = *reinterpret_cast<const float4*>(tl + r * MT_RS + 4 * lane);
    float4 ra[2][4];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            ra[sb][g] = *reinterpret_cast<const float4*>(rb + (4 * sb + (lane & 3)) * MT_ROWS + 4 * g);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wave_lds_sync();
    dma_mtile<AUX>(tl, X, ldx, y, next_row0(), B, lane, yv_cur);
    if (PRIO == 1) __builtin_amdgcn_s_setprio(0);
    if (PRIO == 2) __builtin_amdgcn_s_setprio(1);
    if (DBG == 0 || DBG == 3) {
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r) {
            const float4 xr = x4[r];
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                const float4 rr = ra[sb][r >> 2];
                const float a = (r & 3) == 0 ? rr.x : (r & 3) == 1 ? rr.y : (r & 3) == 2 ? rr.z : rr.w;
                acc[sb][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, xr.x, acc[sb][0], 0, 0, 0);
                acc[sb][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, xr.y, acc[sb][1], 0, 0, 0);
                acc[sb][2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, xr.z, acc[sb][2], 0, 0, 0);
                acc[sb][3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, xr.w, acc[sb][3], 0, 0, 0);
            }
        }
    } else {
        // keep the loads of a deletion build alive
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r) s += x4[r].x;
        if (s == 12345.678f) qacc += ra[0][0].x + ra[1][3].w;
    }
}

// Which tiles a wave of blr_pass_q_kernel reads.
//
// STATIC (reproducible: a wave's tiles and their order are a function of the launch geometry alone).  Window w < n_all
// is one contiguous run of (workgroups x 4) tiles, tile = w * w_all + slot, as in every pass kernel of this file.  The
// workgroups with an EVEN blockIdx then take `n_a - n_all` further windows of (even workgroups x 4) tiles among
// themselves: on this part the XCDs 0, 2, 4, 6 stream 7-15 % faster than 1, 3, 5, 7 (tools/ubench_dma_inflight: the
// same 3 GiB split evenly ends after 390 us on the even XCDs and 450 us on the odd ones), workgroups are dealt to the XCDs
// round-robin, and a pass that gives every workgroup the same share ends when the slow half does.  The placement is an
// observation used for speed only: any placement computes the same sums.
//
// (Measured and dropped: tiles popped from eight atomic queues, one per XCD, with stealing -- every workgroup then ends
// within 0.2 us of every other, but 62 500 returning atomics on eight words take 226 us where the static schedule takes
// 160, profiles/r04_ab_pass_q_schedules.txt; and the sums would no longer be reproducible in the last bits.  Likewise a
// queued tail behind a static share: 0.5-1.5 us of 157 gained, the last bits lost, profiles/r04_ab_pass_q_steal.txt.)
struct QSched {
    int n_all, n_mine, rev, keep;
    int64_t w_all, w_a, slot, slot_a, B;
    __device__ __forceinline__ int64_t row0(int p) const {        // p-th tile of this wave's walk; p >= n_mine: the empty tile
        if (p >= n_mine) return B;
        const int w = rev ? n_mine - 1 - p : p;
        const int64_t tile = w < n_all ? (int64_t)w * w_all + slot
                                       : (int64_t)n_all * w_all + (int64_t)(w - n_all) * w_a + slot_a;
        return tile * MT_ROWS;
    }
};

template <bool NT, int DBG, int PRIO>
__global__ __launch_bounds__(PASS_BLOCK, 2) void blr_pass_q_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_all, int n_a, int rev, int keep,
    unsigned long long* __restrict__ stamps) {
    constexpr int LDS_FLOATS = PASS_WAVES * (MT_WAVE_LDS > SLAB_STRIDE ? MT_WAVE_LDS : SLAB_STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long t_start = stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
    float* tl = lds + wave * MT_WAVE_LDS;
    float* rb = tl + MT_ROWS * MT_RS;          // residuals [draw][row]
    mfma_f32x4 acc[2][4];                      // [draw group][column component]: register i = draw 4 sb + i
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[sb][q] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    float qacc = 0.f;
    float4 yv;
    float wreg[QW];
    // forward B operand: w[draw lane % 8][128 h + 16 k8 + 4 m + c], register 4 (4 h + m) + c; draws >= S are zero
    auto load_w = [&]() {
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
            float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((lane & 7) < S)
                w4 = *reinterpret_cast<const float4*>(W + (int64_t)(lane & 7) * GCOLS + 128 * (c8 >> 2) + 16 * (lane >> 3) +
                                                      4 * (c8 & 3));
            wreg[4 * c8 + 0] = w4.x; wreg[4 * c8 + 1] = w4.y;
            wreg[4 * c8 + 2] = w4.z; wreg[4 * c8 + 3] = w4.w;
        }
    };
    {
        QSched sc;
        sc.n_all = n_all; sc.rev = rev; sc.B = B;
        sc.n_mine = (blockIdx.x & 1) ? n_all : n_a;
        sc.w_all = (int64_t)gridDim.x * PASS_WAVES;
        sc.w_a = (int64_t)((gridDim.x + 1) >> 1) * PASS_WAVES;
        sc.slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
        sc.slot_a = (int64_t)(blockIdx.x >> 1) * PASS_WAVES + wave;
        const int n_mine = sc.n_mine;
        if (!NT) keep = n_mine;
        const int n_stream = n_mine - keep > 0 ? n_mine - keep : 0;   // tiles read non-temporal; the last `keep` allocate
        // the first tile's DMAs go out before anything else: W (L2 hits) loads behind them
        if (n_stream > 0) dma_mtile<2>(tl, X, ldx, y, sc.row0(0), B, lane, yv);
        else dma_mtile<0>(tl, X, ldx, y, sc.row0(0), B, lane, yv);
        load_w();
        int k = 0;
        for (; k + 1 < n_stream; ++k)
            q_tile_step<2, DBG, PRIO>(yv, tl, rb, wreg, acc, qacc, X, ldx, y, [&] { return sc.row0(k + 1); }, B, lane);
        for (; k < n_mine; ++k)
            q_tile_step<0, DBG, PRIO>(yv, tl, rb, wreg, acc, qacc, X, ldx, y, [&] { return sc.row0(k + 1); }, B, lane);
    }
    // no LDS-DMA of this wave may still be in flight when the tile region is reused for the block reduction
    __builtin_amdgcn_s_waitcnt(bsc_vmcnt_only(0));
    __syncthreads();
    float* ep = lds + wave * SLAB_STRIDE;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) slab_chunk_put(ep, lane, 2 * q + sb, acc[sb][q]);   // an accumulator IS a chunk
    float qv = (lane & 8) ? 0.f : qacc;        // lane (draw lane % 8, kq): rows 4 kq .. of that draw; lanes l ^ 8 repeat them
    qv += __shfl_xor(qv, 16);
    qv += __shfl_xor(qv, 32);
    if (lane < SG) ep[SLAB_G + lane] = qv;
    __syncthreads();
    slab_row_out(lds, slab + (int64_t)blockIdx.x * SLAB_STRIDE, tid);
    if (stamps) {
        // measurement aid (option blr_stamps): when did this workgroup start and end, and on which XCD did it run
        // (words 4-7 of a row are unused)
        __syncthreads();
        if (tid == 0) {
            unsigned long long* st = stamps + 8 * (int64_t)blockIdx.x;
            st[0] = t_start;
            st[1] = __builtin_amdgcn_s_memrealtime();
            st[2] = __builtin_amdgcn_s_getreg((3 << 11) | 20);     // HW_REG_XCC_ID[3:0]
            st[3] = __builtin_amdgcn_s_getreg((15 << 11) | 4);     // HW_REG_HW_ID[15:0]
        }
    }
}

// ---- sixteen draws per pass (D == 256, 9 <= S <= 16: bsc_blr_data_pass with S > 8) -------------
//
// One pass over X for 16 draws instead of two.  The tile comes through registers (the prefetched
// NEXT tile: 64 VGPRs), is written to the wave's LDS region row-major and read back twice:
//   forward   A operand of v_mfma_f32_16x16x4_f32: lane (i = l&15, kq = l>>4) reads
//             X[row i][64 kq + 4 j .. +3] (one ds_read_b128 feeds 4 MFMAs); B operand
//             = W[draw l&15][same columns], 64 registers loaded once; result register reg of the
//             lane is dot(row 4 kq + reg, draw l&15): all sixteen MFMA columns carry a draw.
//   backward  the rank-1 updates G[s, :] += r[n, s] x[n, :] on v_mfma_f32_4x4x1_16B_f32 -- sixteen
//             independent 4 x 4 outer products per instruction: block b = lane / 4 owns columns
//             16 b .. 16 b + 15, the A operand is the residual r[n][4 sb + lane % 4] (the same in
//             every block), the B operand component q of the row as the lane holds it (column
//             4 lane + q), and the result register i of accumulator (sb, q) is
//             G[4 sb + i][4 lane + q] -- the accumulators the VALU kernel keeps, so the epilogue and
//             the slab layout are unchanged.
//
// Schedule (`Sched`).  Iteration k of every wave reads one contiguous WINDOW of gridDim.x * 4 tiles
// (33 MB at 1M x 256 on 505 workgroups); `rev` walks the windows from the end of the mini-batch to
// its start.  The last `keep` windows of a sweep are read with the allocating cache policy,
// everything before them non-temporal: they are then still in the 256 MiB Infinity Cache when the
// NEXT sweep over the same mini-batch -- run in the other direction -- starts with exactly those
// windows.
struct Sched {
    int n_iter, rev, keep;
    int64_t stride0, slot, B;
    __device__ __forceinline__ int window(int p) const { return rev ? n_iter - 1 - p : p; }
    // allocating policy for the window at position p?  (p = n_iter: the empty prefetch after the last)
    __device__ __forceinline__ bool kept(int p) const { return p >= n_iter - keep; }
    __device__ __forceinline__ int64_t row0(int p) const {
        return p < n_iter ? ((int64_t)window(p) * stride0 + slot) * MT_ROWS : B;
    }
};

constexpr int MX_WAVE_LDS = MT_ROWS * MT_RS + MT_ROWS * 16;   // tile + residuals of up to 16 draws

// NSB = draw groups of four per pass: 4 is the only instantiation (the forward is the same for any
// NSB <= 4, the backward's cost is proportional to it).  The block partials of draws 8 .. 15 go to a
// second slab behind the first (slab + gridDim.x rows).
template <bool NT, int NSB>
__global__ __launch_bounds__(PASS_BLOCK, 2) void blr_pass_mx_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter, int rev, int keep) {
    constexpr int NS = 4 * NSB;                 // draws per pass
    constexpr int NH = NSB / 2;                 // slabs (one per eight draws)
    constexpr int LDS_FLOATS = PASS_WAVES * (MX_WAVE_LDS > NH * SLAB_STRIDE ? MX_WAVE_LDS : NH * SLAB_STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* tl = lds + wave * MX_WAVE_LDS;      // this wave's tile
    float* rb = tl + MT_ROWS * MT_RS;          // residuals [sample][row]

    // forward B operand: W[draw i16][64 kq + 4 j + c]; draws >= S are zero.  Lane group kq contracts
    // columns 64 kq .. 64 kq + 63, so the four 16-byte A reads of a row lie 256 B apart on the same
    // banks and each ds_read_b128 lane group (all 16 rows once, two different kq) is conflict-free;
    // interleaved columns (16 j + 4 kq) gave every lane group a 2-way conflict.
    float wreg[GCOLS / 4];
#pragma unroll
    for (int j = 0; j < GCOLS / 16; ++j) {
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i16 < S) w4 = *reinterpret_cast<const float4*>(W + (int64_t)i16 * GCOLS + 64 * kq + 4 * j);
        wreg[4 * j + 0] = w4.x; wreg[4 * j + 1] = w4.y;
        wreg[4 * j + 2] = w4.z; wreg[4 * j + 3] = w4.w;
    }
    mfma_f32x4 acc[NSB][4];                    // [sample group][column component]: register i = sample 4 sb + i
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[sb][q] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    float qacc = 0.f;
    const bool live = i16 < NS;                // lanes whose forward MFMA column is a sample

    Sched sc;
    sc.n_iter = n_iter; sc.rev = rev; sc.keep = NT ? keep : n_iter;
    sc.stride0 = (int64_t)gridDim.x * PASS_WAVES;
    sc.slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
    sc.B = B;

    MTile t;
    if (sc.kept(0)) load_mtile_policy<0>(t, X, ldx, y, sc.row0(0), B, lane);
    else load_mtile_policy<2>(t, X, ldx, y, sc.row0(0), B, lane);
    for (int p = 0; p < n_iter; ++p) {
        // the tile to LDS, its registers take the next window's tile (tiles outside the mini-batch
        // read zeros without touching memory)
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r)
            *reinterpret_cast<float4*>(tl + r * MT_RS + 4 * lane) = t.x[r];
        const float4 yv = t.yv;
        const int64_t next0 = sc.row0(p + 1);
        if (sc.kept(p + 1)) load_mtile_policy<0>(t, X, ldx, y, next0, B, lane);
        else load_mtile_policy<2>(t, X, ldx, y, next0, B, lane);
        wave_lds_sync();

        // forward on v_mfma_f32_16x16x4_f32 (two accumulators, no MFMA waits on its predecessor)
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
        // result register reg of lane (i16, kq) = dot(row 4 kq + reg, sample i16); the residuals go
        // to rb[sample][row]: one 16-byte store per live lane
        if (live) {
            const float r0 = yv.x - (d0[0] + d1[0]), r1 = yv.y - (d0[1] + d1[1]);
            const float r2 = yv.z - (d0[2] + d1[2]), r3 = yv.w - (d0[3] + d1[3]);
            qacc = fmaf(r0, r0, qacc); qacc = fmaf(r1, r1, qacc);
            qacc = fmaf(r2, r2, qacc); qacc = fmaf(r3, r3, qacc);
            *reinterpret_cast<float4*>(rb + i16 * MT_ROWS + 4 * kq) = make_float4(r0, r1, r2, r3);
        }
        wave_lds_sync();

        // backward on v_mfma_f32_4x4x1_16B_f32: per row NSB draw groups x 4 column components
#pragma unroll
        for (int g = 0; g < MT_ROWS / 4; ++g) {
            if (g) asm volatile("" ::: "memory");   // four rows of reads in flight
            // A operands of rows 4 g .. 4 g + 3: r[row][4 sb + lane % 4] (broadcast reads)
            float4 ra[NSB];
#pragma unroll
            for (int sb = 0; sb < NSB; ++sb)
                ra[sb] = *reinterpret_cast<const float4*>(rb + (4 * sb + (lane & 3)) * MT_ROWS + 4 * g);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float4 x4 = *reinterpret_cast<const float4*>(tl + (4 * g + rr) * MT_RS + 4 * lane);
#pragma unroll
                for (int sb = 0; sb < NSB; ++sb) {
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

    // block reduction through LDS, fixed order over waves (slab layout of the other pass kernels,
    // one slab per eight draws)
    __syncthreads();
    float* ep = lds + wave * (NH * SLAB_STRIDE);
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(ep + (sb >> 1) * SLAB_STRIDE + (4 * (sb & 1) + i) * GCOLS + 4 * lane) =
                make_float4(acc[sb][0][i], acc[sb][1][i], acc[sb][2][i], acc[sb][3][i]);
    float qv = live ? qacc : 0.f;              // lane (i16, kq): rows 4 kq .. of draw i16
    qv += __shfl_xor(qv, 16);
    qv += __shfl_xor(qv, 32);
    if (lane < NS) ep[(lane >> 3) * SLAB_STRIDE + SLAB_G + (lane & 7)] = qv;
    __syncthreads();
    for (int i = tid; i < NH * SLAB_STRIDE; i += PASS_BLOCK) {
        const int h = i / SLAB_STRIDE, ii = i - h * SLAB_STRIDE;
        const int src = h * SLAB_STRIDE + (ii < SLAB_G ? (ii & 7) * GCOLS + (ii >> 3) : ii);
        float v = lds[src];
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) v += lds[k * (NH * SLAB_STRIDE) + src];
        slab[((int64_t)h * gridDim.x + blockIdx.x) * SLAB_STRIDE + ii] = v;
    }
}

__global__ __launch_bounds__(RED_BLOCK) void blr_slab_reduce_kernel(
    const float* __restrict__ slab, int n_blocks, int D, int S, int s_base,
    double* __restrict__ Q, double* __restrict__ G) {
    regress_slab_reduce(slab, n_blocks, D, S, s_base, Q, G);
}

// ---- sampler and ELBO/gradient finish (tiny, float64) ----------------------

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

#pragma clang fp contract(off)
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint32_t block, uint32_t sample,
                                               uint32_t stream, uint32_t step, double (&z)[4]) {
    uint32_t c[4] = {block, sample, stream, step};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double two_m32 = 2.3283064365386963e-10;  // 2^-32
    const double two_pi = 6.283185307179586476925286766559;
    double u0 = ((double)c[0] + 0.5) * two_m32;
    double u1 = ((double)c[1] + 0.5) * two_m32;
    double u2 = ((double)c[2] + 0.5) * two_m32;
    double u3 = ((double)c[3] + 0.5) * two_m32;
    double r0 = sqrt(-2.0 * log(u0));
    double r1 = sqrt(-2.0 * log(u2));
    double t0 = two_pi * u1;
    double t1 = two_pi * u3;
    z[0] = r0 * cos(t0);
    z[1] = r0 * sin(t0);
    z[2] = r1 * cos(t1);
    z[3] = r1 * sin(t1);
}

__global__ void philox_normal_kernel(uint64_t seed, uint32_t stream, uint32_t step,
                                     int n_samples, int n_params, double* __restrict__ eps) {
    const int n_blocks = (n_params + 3) / 4;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_samples * n_blocks) return;
    const int s = idx / n_blocks, b = idx % n_blocks;
    double z[4];
    philox_normal4(seed, (uint32_t)b, (uint32_t)s, stream, step, z);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * b + j < n_params) eps[(int64_t)s * n_params + 4 * b + j] = z[j];
}

// eps for `n_steps` consecutive Philox steps in one launch:
// eps[(k*S + s)*(D+1) + d], d < D from stream 0, d == D from stream 1 (the layout
// bsc_blr_sample writes for one step).  The noise does not depend on the
// parameters, so it is produced ahead of time and kept out of the update's
// latency chain.
__global__ void blr_noise_kernel(int D, int S, uint64_t seed, uint32_t step0, int n_steps,
                                 double* __restrict__ eps) {
    const int n_blocks = (D + 3) / 4;
    const int per_step = S * n_blocks + S;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)per_step * n_steps) return;
    const int k = (int)(idx / per_step), r = (int)(idx % per_step);
    double* out = eps + (int64_t)k * S * (D + 1);
    double z[4];
    if (r < S * n_blocks) {
        const int s = r / n_blocks, b = r % n_blocks;
        philox_normal4(seed, (uint32_t)b, (uint32_t)s, 0u, step0 + (uint32_t)k, z);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * b + j < D) out[(int64_t)s * (D + 1) + 4 * b + j] = z[j];
    } else {
        const int s = r - S * n_blocks;
        philox_normal4(seed, 0u, (uint32_t)s, 1u, step0 + (uint32_t)k, z);
        out[(int64_t)s * (D + 1) + D] = z[0];
    }
}

// Draws for Philox block `pb` (columns 4pb..4pb+3) of sample s, given m, rho
// indexed by absolute column.
__device__ __forceinline__ void blr_draw_block(const double* m, const double* rho, int D, int s,
                                               int pb, uint64_t seed, uint32_t step,
                                               double* __restrict__ eps, float* __restrict__ W) {
    double z[4];
    philox_normal4(seed, (uint32_t)pb, (uint32_t)s, 0u, step, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = 4 * pb + j;
        if (d < D) {
            eps[(int64_t)s * (D + 1) + d] = z[j];
            double sd = exp(rho[d]);
            double wv = m[d] + sd * z[j];
            W[(int64_t)s * D + d] = (float)wv;
        }
    }
}

__device__ __forceinline__ void blr_draw_scale(double a, double b, int D, int s, uint64_t seed,
                                               uint32_t step, double* __restrict__ eps,
                                               double* __restrict__ xi) {
    double z[4];
    philox_normal4(seed, 0u, (uint32_t)s, 1u, step, z);
    eps[(int64_t)s * (D + 1) + D] = z[0];
    double sd = exp(b);
    xi[s] = a + sd * z[0];
}

__global__ void blr_sample_kernel(const double* __restrict__ lam, int D, int S, uint64_t seed,
                                  uint32_t step, double* __restrict__ eps,
                                  float* __restrict__ W, double* __restrict__ xi) {
    const int n_blocks = (D + 3) / 4;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < S * n_blocks) {
        blr_draw_block(lam, lam + D, D, idx / n_blocks, idx % n_blocks, seed, step, eps, W);
    } else if (idx < S * n_blocks + S) {
        blr_draw_scale(lam[2 * D], lam[2 * D + 1], D, idx - S * n_blocks, seed, step, eps, xi);
    }
}

// One workgroup.  Thread d owns column d (strided when D > blockDim).
constexpr int FIN_BLOCK = 256;
constexpr int FIN_WAVES = FIN_BLOCK / BSC_WAVE;
constexpr int FIN_MAX_S = 64;

__global__ __launch_bounds__(FIN_BLOCK) void blr_elbo_grad_kernel(
    const double* __restrict__ lam, const double* __restrict__ eps,
    const float* __restrict__ W, const double* __restrict__ xi, const double* __restrict__ Q,
    const double* __restrict__ G, int D, int S, double batch_rows, double scale, double alpha0,
    double beta0, double* __restrict__ elbo, double* __restrict__ grad) {
    __shared__ double red[FIN_WAVES][FIN_MAX_S + 1];
    __shared__ double wsq[FIN_MAX_S];
    __shared__ double e_inv[FIN_MAX_S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // |w_s|^2 for every sample and sum(rho), fixed-order block reduction
    for (int s = 0; s <= S; ++s) {
        double part = 0.0;
        for (int d = tid; d < D; d += FIN_BLOCK) {
            if (s < S) {
                double wv = (double)W[(int64_t)s * D + d];
                part += wv * wv;
            } else {
                part += lam[D + d];
            }
        }
        part = wave_allsum_f64(part);
        if (lane == 0) red[wave][s] = part;
    }
    __syncthreads();
    if (tid < S) {
        double t = 0.0;
        for (int k = 0; k < FIN_WAVES; ++k) t += red[k][tid];
        wsq[tid] = t;
        e_inv[tid] = exp(-xi[tid]);
    }
    __syncthreads();

    const double inv_S = 1.0 / (double)S;
    for (int d = tid; d < D; d += FIN_BLOCK) {
        double gm = 0.0, gr = 0.0;
        for (int s = 0; s < S; ++s) {
            double wv = (double)W[(int64_t)s * D + d];
            double dw = e_inv[s] * (scale * G[(int64_t)s * D + d] - wv);
            gm += dw;
            gr += dw * eps[(int64_t)s * (D + 1) + d];
        }
        grad[d] = gm * inv_S;
        grad[D + d] = gr * inv_S * exp(lam[D + d]) + 1.0;
    }
    if (tid == 0) {
        double sum_rho = 0.0;
        for (int k = 0; k < FIN_WAVES; ++k) sum_rho += red[k][S];
        const double b = lam[2 * D + 1];
        double fa = 0.0, fb = 0.0, fsum = 0.0;
        for (int s = 0; s < S; ++s) {
            const double e = e_inv[s], x = xi[s];
            double dxi = -0.5 * (scale * batch_rows + (double)D) - alpha0 +
                         e * (0.5 * scale * Q[s] + 0.5 * wsq[s] + beta0);
            fa += dxi;
            fb += dxi * eps[(int64_t)s * (D + 1) + D];
            double loglik = scale * (-0.5 * batch_rows * (BSC_LOG_2PI + x) - 0.5 * e * Q[s]);
            double logpw = -0.5 * (double)D * (BSC_LOG_2PI + x) - 0.5 * e * wsq[s];
            double logpxi = alpha0 * log(beta0) - lgamma(alpha0) - alpha0 * x - beta0 * e;
            fsum += loglik + logpw + logpxi;
        }
        grad[2 * D] = fa * inv_S;
        grad[2 * D + 1] = fb * inv_S * exp(b) + 1.0;
        elbo[0] = fsum * inv_S + sum_rho + b + 0.5 * (double)(D + 1) * (1.0 + BSC_LOG_2PI);
    }
}

// ---- fused finish: slab reduce + ELBO/gradient + Adam + next draw ----------
//
// Grid = ceil(D/8) column workgroups + 1 scalar workgroup.  A column workgroup
// owns 8 columns x S<=8 samples (one 256-B run per slab row); the scalar
// workgroup owns Q, |w_s|^2, the entropy term, (a, b) and the ELBO.  State is
// double-buffered by the caller (lam_in/lam_out, cur/next draws) so no
// workgroup reads what another one writes.

struct FusedArgs {
    const float* slab;     // block partials of the pass kernel, or nullptr
    int n_slab;            // slab rows
    const double* stats;   // [Q (S) | G (S*D)] when slab == nullptr
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;
    const float* W;
    const double* xi;
    double* eps_next;      // nullptr: no next draw
    int eps_next_ready;    // 1: eps_next already holds the noise of next_step (bsc_blr_noise)
    float* W_next;
    double* xi_next;
    double* elbo;
    double* grad;
    int D, S;
    // the log-joint per draw as a member of the family (bsc_blr_fused_update_general):
    //   f(w, xi; Q) = c0 + c_xi xi + e^{-xi} (-s_q Q / 2 - k_w |w|^2 / 2 - beta)
    double c0, c_xi, s_q, k_w, beta;
    bsc_adam adam;
    uint64_t seed;
    uint32_t next_step;
    unsigned long long* stamps;   // option blr_finish_stamps: FIN_STAMPS words per workgroup, else nullptr
};

// Stage stamps of the finish (measurement aid, option blr_finish_stamps; the STAMP instantiations only, so the kernel
// that ships carries none of it).  Thread 0 of a workgroup keeps one s_memrealtime per stage and writes them at its end:
//   0 wave start | 1 small operands landed | 2 slab landed and summed | 3 after the workgroup barrier |
//   4, 5 scalar workgroup: per-draw terms handed over through LDS / their fixed-order sums done |
//   6 Adam done | 7 stores issued | 8 end
// A stage a workgroup does not have repeats the stage before it.
constexpr int FIN_STAMPS = 16;           // words per workgroup (two 64-byte rows of bsc_blr_read_stamps)
constexpr int FIN_STAMP_WGS = 64;        // workgroups that fit the stamp buffer behind the pass's rows

template <bool STAMP>
struct FinStamps {
    unsigned long long t[9];
    __device__ __forceinline__ void at(int k) {
        if (STAMP) t[k] = __builtin_amdgcn_s_memrealtime();
    }
    // every load issued before the last `behind` ones has landed (loads return in order)
    template <int BEHIND>
    __device__ __forceinline__ void landed(int k) {
        if (STAMP) {
            __builtin_amdgcn_s_waitcnt(bsc_vmcnt_only(BEHIND));
            asm volatile("" ::: "memory");
            at(k);
        }
    }
    __device__ __forceinline__ void skip(int k) {
        if (STAMP) t[k] = t[k - 1];
    }
    __device__ __forceinline__ void write(unsigned long long* stamps) {
        if (STAMP && threadIdx.x == 0 && (int)blockIdx.x < FIN_STAMP_WGS) {
            at(8);
            unsigned long long* st = stamps + FIN_STAMPS * (int64_t)blockIdx.x;
#pragma unroll
            for (int k = 0; k < 9; ++k) st[k] = t[k];
        }
    }
};

// slab_column_sum (csrc/bsc_regress.h) of slab column `col` with a hook and without branches: `between` runs once, after
// the first batch of loads has been issued and before it is consumed, and the loads are buffer loads whose descriptor
// ends with the slab -- a row past n_rows reads as zero, where the guarded load of slab_column_sum is a branch that waits
// for its load (eight round trips in a row).  The same values and the same order of additions.
template <int STRIDE, int BATCH, typename F>
__device__ __forceinline__ double slab_column_sum_between(const float* __restrict__ slab, int col, int first, int step,
                                                          int n_rows, F between) {
    const uint64_t slab_bytes = (uint64_t)n_rows * STRIDE * 4u;
    auto rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)slab, 0, slab_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)slab_bytes, 0x00020000);
    double sum = 0.0;
    bool pending = true;
    for (int b0 = first; b0 < n_rows; b0 += step * BATCH) {
        float v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j)
            v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, ((b0 + j * step) * STRIDE + col) * 4, 0, 0));
        if (pending) { between(); pending = false; }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) sum += (double)v[j];
    }
    if (pending) between();
    return sum;
}

// BLOCK threads per workgroup (1024 = 16 waves: 32 slab rows per wave at 512 partials; fewer waves
// launch sooner -- BSC_BLR_FINISH_BLOCK, A/B in tools/ab_pass.py)
template <int FUSED_BLOCK, bool STAMP>
__global__ __launch_bounds__(FUSED_BLOCK) void blr_fused_update_kernel(FusedArgs a) {
    constexpr int FUSED_WAVES = FUSED_BLOCK / BSC_WAVE;
    constexpr int SLAB_JJ = FUSED_WAVES >= 16 ? 8 : 32;      // slab loads a lane has in flight (slab_run_sum)
    constexpr int Q_BATCH = FUSED_BLOCK >= 1024 ? 8 : 16;    // the same for the scalar workgroup's column of Q
    __shared__ double red[FUSED_WAVES][BSC_WAVE];
    __shared__ double sh[2 * FIN_MAX_S + 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: branches on it are scalar
    FinStamps<STAMP> stamp;
    stamp.at(0);
    const int D = a.D, S = a.S;
    const int n_chunks = (D + 7) / 8;
    const int chunk = (int)blockIdx.x;   // == n_chunks: the scalar workgroup
    const double inv_S = 1.0 / (double)S;

    if (chunk < n_chunks) {
        // ---------------- column workgroup: columns d0 .. d0+7 ----------------
        const int d0 = 8 * chunk;
        const int dl = lane >> 3, sl = lane & 7;  // slab order within the run is [d][s]
        const int d = d0 + dl;
        double gm = 0.0, gr = 0.0;
        // every small operand of wave 0 is requested before the slab so that the whole
        // workgroup pays one memory round trip, not one per dependent stage.  The loads are
        // UNCONDITIONAL, from clamped indices: a load under a lane condition is waited for
        // (s_waitcnt vmcnt(0)) where its branch ends, so every such block was a round trip of
        // its own and the slab was asked for last.  A lane outside the condition reads a
        // neighbour's value and never uses it.
        double p_m = 0.0, p_rho = 0.0, p_m1 = 0.0, p_m2 = 0.0, p_r1 = 0.0, p_r2 = 0.0;
        double e_next = 0.0, e_rho = 0.0;   // e_rho = exp(rho), set before it is used on either path
        const bool pre_noise = a.eps_next && a.eps_next_ready;
        const int dc = d < D ? d : D - 1, sc = sl < S ? sl : S - 1;
        if (wave == 0) {
            p_m = a.lam_in[dc]; p_rho = a.lam_in[D + dc];
            p_m1 = a.m1[dc]; p_m2 = a.m2[dc];
            p_r1 = a.m1[D + dc]; p_r2 = a.m2[D + dc];
            if (pre_noise) e_next = a.eps_next[(int64_t)sc * (D + 1) + dc];
        }
        if (a.slab) {  // S <= 8: lane <-> (column dl, sample sl) of one 256-B slab run
            const bool live = sl < S && d < D;
            float wf = 0.f;   // (widened where it is used: a conversion here would wait for the load)
            double xs = 0.0, ev = 0.0;
            if (wave == 0) {
                wf = a.W[(int64_t)sc * D + dc];
                xs = a.xi[sc];
                ev = a.eps[(int64_t)sc * (D + 1) + dc];
            }
            // this wave's share of the slab (rows wave + 16 k, the workgroup's 64-float run); the
            // float64 exponentials that do not depend on it run while it is in flight
            double s4[4];
            double e_mxs = 0.0;
            slab_run_sum<SLAB_STRIDE, FUSED_WAVES, SLAB_JJ>(a.slab, a.n_slab, 64 * chunk, wave, lane, s4, [&] {
                stamp.template landed<SLAB_JJ>(1);
                if (wave == 0) {
                    e_mxs = exp(-xs);
                    e_rho = exp(p_rho);
                }
            });
            stamp.at(2);
            if (lane < 16) {
#pragma unroll
                for (int i = 0; i < 4; ++i) red[wave][4 * lane + i] = s4[i];
            }
            __syncthreads();
            if (wave != 0) return;
            stamp.at(3);
            double g = red[0][lane];
#pragma unroll
            for (int k = 1; k < FUSED_WAVES; ++k) g += red[k][lane];
            if (live) {
                asm volatile("" : "+v"(wf));   // (keeps the compiler from hoisting the conversion back to the load)
                const double wv = (double)wf;
                const double dw = e_mxs * (a.s_q * g - a.k_w * wv);
                gm = dw;
                gr = dw * ev;
            }
        } else {
            if (wave != 0) return;
            stamp.template landed<0>(1);
            stamp.skip(2);
            stamp.skip(3);
            e_rho = exp(p_rho);
            for (int s = sl; s < S; s += 8) {
                if (d < D) {
                    const double g = a.stats[S + (int64_t)s * D + d];
                    const double wv = (double)a.W[(int64_t)s * D + d];
                    const double dw = exp(-a.xi[s]) * (a.s_q * g - a.k_w * wv);
                    gm += dw;
                    gr += dw * a.eps[(int64_t)s * (D + 1) + d];
                }
            }
        }
        // fold the 8 sample lanes (lane bits 0-2)
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            gm += __shfl_xor(gm, off);
            gr += __shfl_xor(gr, off);
        }
        double* new_m = sh;        // [8]
        double* new_rho = sh + 8;  // [8]
        // the two Adam steps of a column side by side: lane sl = 0 steps m, lane sl = 1 steps rho (every lane of the
        // column holds both gradients after the fold and, the loads being unconditional, both parameters' state)
        if (sl < 2 && d < D) {
            const bool r = sl == 1;
            const double g_m = gm * inv_S;
            const double g_r = gr * inv_S * e_rho + 1.0;
            const double g = r ? g_r : g_m;
            double m1 = r ? p_r1 : p_m1, m2 = r ? p_r2 : p_m2;
            const double np = bsc_adam_ascent(r ? p_rho : p_m, g, m1, m2, a.adam);
            const int at = r ? D + d : d;
            a.grad[at] = g;
            a.m1[at] = m1; a.m2[at] = m2;
            a.lam_out[at] = np;
            (r ? new_rho : new_m)[dl] = np;
        }
        stamp.skip(4);
        stamp.skip(5);
        stamp.at(6);
        wave_lds_sync();
        if (pre_noise) {
            // noise precomputed: w = m + e^rho * eps for this lane's (column, sample)
            for (int s = sl; s < S; s += 8)
                if (d < D) {
                    const double sd = exp(new_rho[dl]);
                    const double en = s == sl ? e_next : a.eps_next[(int64_t)s * (D + 1) + d];
                    a.W_next[(int64_t)s * D + d] = (float)(new_m[dl] + sd * en);
                }
        } else if (a.eps_next) {
            // two Philox blocks per sample cover the 8 columns
            for (int i = lane; i < 2 * S; i += BSC_WAVE) {
                const int s = i >> 1, pb = 2 * chunk + (i & 1);
                if (4 * pb < D)
                    blr_draw_block(new_m - d0, new_rho - d0, D, s, pb, a.seed, a.next_step,
                                   a.eps_next, a.W_next);
            }
        }
        stamp.at(7);
        stamp.write(a.stamps);
        return;
    }

    // ---------------------------- scalar workgroup ----------------------------
    double* Qs = sh;                    // [S]
    double* wsq = sh + FIN_MAX_S;       // [S]
    double* misc = sh + 2 * FIN_MAX_S;  // [0]=sum of rho
    __shared__ double terms[3 * FIN_MAX_S];
    const bool pre_noise = a.eps_next && a.eps_next_ready;
    // request every small operand first (one memory round trip for the workgroup): unconditional loads from clamped
    // indices, as in the column workgroups -- a thread past the range reads a neighbour's value and never uses it
    const int sc = tid < S ? tid : S - 1;                 // thread s < S
    const double x_s = a.xi[sc];
    const double e_sD = a.eps[(int64_t)sc * (D + 1) + D];
    double e_next = 0.0;
    if (pre_noise) e_next = a.eps_next[(int64_t)sc * (D + 1) + D];
    // the two scalar parameters, one lane each: thread 0 owns a, thread 1 owns b (value and Adam moments); thread 2,
    // which writes the ELBO, needs b as well
    const int pc = tid < 1 ? 0 : 1;
    double p_v = a.lam_in[2 * D + pc], p_1 = a.m1[2 * D + pc], p_2 = a.m2[2 * D + pc];
    const double bv = a.lam_in[2 * D + 1];
    // the float64 exponentials that depend on the small operands alone run while the slab is in flight
    double e_mx = 0.0, e_pv = 0.0;                         // exp(-xi_s) (thread s < S), exp(b) (thread 1)
    auto early_exps = [&] {
        if (wave == 0) {
            e_mx = exp(-x_s);
            e_pv = exp(p_v);
        }
    };
    // the sum of rho: this thread's first term is requested here and added behind the slab loads -- a loop that adds
    // as it loads waits for memory before the slab has even been asked for (a second round trip on the chain)
    const double rho_pre = a.lam_in[D + (tid < D ? tid : D - 1)];
    // |w_s|^2: wave-per-sample, fixed order (first 4 loads of each lane issued here)
    float wpre[4];
    {
        const int ws = wave < S ? wave : S - 1;    // (used where wave < S and d < D)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = lane + BSC_WAVE * j;
            wpre[j] = a.W[(int64_t)ws * D + (d < D ? d : D - 1)];
        }
    }
    if (a.slab) {  // S <= 8: thread -> (sample tid&7, slab-row group tid>>3)
        double part = slab_column_sum_between<SLAB_STRIDE, Q_BATCH>(a.slab, SLAB_G + (tid & 7), tid >> 3, FUSED_BLOCK / 8,
                                                                    a.n_slab, [&] {
                                                                        stamp.template landed<Q_BATCH>(1);
                                                                        early_exps();
                                                                    });
        // fold the 8 row groups of this wave (lane bits 3-5), then the 16 waves
        part += __shfl_xor(part, 8);
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (lane < 8) red[wave][lane] = part;
        stamp.at(2);
    } else {
        for (int s = tid; s < S; s += FUSED_BLOCK) Qs[s] = a.stats[s];
        stamp.template landed<0>(1);
        stamp.skip(2);
        early_exps();
    }
    for (int s = wave; s < S; s += FUSED_WAVES) {
        double part = 0.0;
        int d = lane;
        if (s == wave) {  // the prefetched columns, same ascending order as the loop below
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (d < D) part += (double)wpre[j] * (double)wpre[j];
                d += BSC_WAVE;
            }
        }
        for (; d < D; d += BSC_WAVE) {
            const double wv = (double)a.W[(int64_t)s * D + d];
            part += wv * wv;
        }
        part = wave_allsum_f64(part);
        if (lane == 0) wsq[s] = part;
    }
    double rho_part = 0.0;
    if (tid < D) rho_part += rho_pre;          // the same terms in the same ascending order
    for (int d = tid + FUSED_BLOCK; d < D; d += FUSED_BLOCK) rho_part += a.lam_in[D + d];
    rho_part = wave_allsum_f64(rho_part);
    if (lane == 0) red[wave][32] = rho_part;  // column 32: clear of the Q staging columns
    __syncthreads();
    // What is left is one wave's work: the other waves are done, and wave 0 hands its values from lane to lane through
    // LDS behind wave-level fences -- no second or third workgroup barrier on the chain.
    if (wave != 0) return;
    stamp.at(3);
    // lane l adds column l of the staging rows in wave order: lanes 0-7 end with Q, lane 32 with the sum of rho (the
    // other columns are not read again)
    double colsum = 0.0;
    for (int k = 0; k < FUSED_WAVES; ++k) colsum += red[k][lane];
    if (lane == 32) misc[0] = colsum;
    // per-sample terms in parallel (one lane per sample), then fixed-order sums
    double* t_dxi = terms;              // [S]
    double* t_dxe = t_dxi + FIN_MAX_S;  // [S]
    double* t_f = t_dxe + FIN_MAX_S;    // [S]
    if (lane < S) {
        const int s = lane;
        const double Qv = a.slab ? colsum : Qs[s];
        const double x = x_s, e = e_mx;
        const double inner = 0.5 * a.s_q * Qv + 0.5 * a.k_w * wsq[s] + a.beta;
        const double dxi = a.c_xi + e * inner;
        t_dxi[s] = dxi;
        t_dxe[s] = dxi * e_sD;
        t_f[s] = a.c0 + a.c_xi * x - e * inner;
    }
    wave_lds_sync();
    stamp.at(4);
    // lane 0: sum of dxi (the gradient of a), lane 1: sum of dxi * eps (of b), lane 2: sum of f (the ELBO) -- each
    // from s = 0 upwards, as one thread used to add all three
    double f = 0.0;
    if (lane < 3) {
        const double* t = terms + lane * FIN_MAX_S;
        for (int s = 0; s < S; ++s) f += t[s];
    }
    stamp.at(5);
    double np_v = 0.0;                  // lane 0: new a, lane 1: new b
    if (lane == 2) a.elbo[0] = f * inv_S + misc[0] + bv + 0.5 * (double)(D + 1) * (1.0 + BSC_LOG_2PI);
    if (lane < 2) {
        double g = f * inv_S;
        if (lane == 1) g = g * e_pv + 1.0;
        a.grad[2 * D + lane] = g;
        np_v = bsc_adam_ascent(p_v, g, p_1, p_2, a.adam);
        a.m1[2 * D + lane] = p_1;
        a.m2[2 * D + lane] = p_2;
        a.lam_out[2 * D + lane] = np_v;
    }
    stamp.at(6);
    // the next xi in the lanes that hold its noise
    const double na = __shfl(np_v, 0), nb = __shfl(np_v, 1);
    if (pre_noise) {
        if (lane < S) a.xi_next[lane] = na + exp(nb) * e_next;
    } else if (a.eps_next) {
        if (lane < S) blr_draw_scale(na, nb, D, lane, a.seed, a.next_step, a.eps_next, a.xi_next);
    }
    stamp.at(7);
    stamp.write(a.stamps);
}

// Tile height of the variant that will run: 16 = forward on the MFMA pipe (needs the full
// 256-column layout and 16-byte aligned y), else the VALU kernel with 8- or 4-row tiles.
int pass_rows(const bsc_ctx* ctx, int D, const float* y) {
    if (ctx->blr_tile_rows == 16)
        return (D == GCOLS && (((uintptr_t)y) & 15) == 0) ? 16 : 8;
    return ctx->blr_tile_rows;
}

// The grid for tiles of `rows` rows at the occupancy of the kernel that runs them (capped by blr_waves_per_simd).
PassGrid blr_pass_grid(const bsc_ctx* ctx, int64_t B, int rows) {
    int occ = rows == 4 ? Geo<4>::OCC : 2;
    if (ctx->blr_waves_per_simd > 0 && ctx->blr_waves_per_simd < occ) occ = ctx->blr_waves_per_simd;
    return pass_grid(ctx, B, rows, occ);
}

constexpr int MAX_SLAB_ROWS = 4 * 256 + 64;  // workspace sizing hint for callers

// The stamp buffer of options blr_stamps / blr_finish_stamps: 64 bytes per pass workgroup, then the finish's rows.
bool stamp_buffer(bsc_ctx* ctx) {
    constexpr size_t bytes = ((size_t)MAX_SLAB_ROWS + (size_t)FIN_STAMP_WGS * (FIN_STAMPS / 8)) * 64;
    if (!ctx->stamps && hipMalloc(&ctx->stamps, bytes) != hipSuccess) ctx->stamps = nullptr;
    return ctx->stamps != nullptr;
}

// Every pass entry point reports under the name of bsc_blr_data_pass.
int check_pass_args(const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                    const float* W, int32_t S, int max_s) {
    BSC_REQUIRE(y || B <= 0, "bsc_blr_data_pass: null pointer");
    return check_regress_args("bsc_blr_data_pass", X, ldx, B, D, W, S, max_s);
}

template <int ROWS, bool NT>
void launch_pass_rows(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B,
                      int D, const float* W, int sg, PassGrid g, float* slab) {
    if (D == GCOLS)
        hipLaunchKernelGGL((blr_pass_kernel<true, ROWS, NT>), dim3(g.n_blocks), dim3(PASS_BLOCK), 0,
                           ctx->stream, X, ldx, y, B, D, W, sg, slab, g.n_iter);
    else
        hipLaunchKernelGGL((blr_pass_kernel<false, ROWS, NT>), dim3(g.n_blocks), dim3(PASS_BLOCK),
                           0, ctx->stream, X, ldx, y, B, D, W, sg, slab, g.n_iter);
}

// Windows (one per iteration: n_blocks * 4 tiles of 16 rows) that fit the Infinity Cache.
int keep_windows(const bsc_ctx* ctx, int64_t ldx, PassGrid g) {
    if (ctx->blr_keep >= 0) return ctx->blr_keep < g.n_iter ? ctx->blr_keep : g.n_iter;
    const double window = (double)g.n_blocks * PASS_WAVES * MT_ROWS * (double)ldx * 4.0;
    // MI355X_MICROARCH.md: Infinity Cache 256 MiB; y, the slab and the draws live there too, and
    // tools/ab_pass.py sweep measures 6-8 windows of 33 MB best, 9-10 worse: aim at 7/8 of it
    const double cache = 224.0 * 1024.0 * 1024.0;
    int k = window > 0 ? (int)(cache / window + 0.5) : 0;
    return k < g.n_iter ? k : g.n_iter;
}

// sweep: BSC_SWEEP_STREAM (0) forward, every load non-temporal; BSC_SWEEP_FORWARD_KEEP (1) forward,
// BSC_SWEEP_BACKWARD_KEEP (2) backward, the windows read last left in the Infinity Cache.  The 4-
// and 8-row kernels (D != 256) always stream forward.
void launch_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int D,
                 const float* W, int sg, PassGrid g, float* slab, int sweep, bool wide = false) {
    const bool nt = ctx->blr_nt_loads != 0;
    const int rows = pass_rows(ctx, D, y);
    bsc_prof_scope prof(ctx);  // times the pass kernel alone
    const int rev = sweep == BSC_SWEEP_BACKWARD_KEEP ? 1 : 0;
    const int keep = sweep == BSC_SWEEP_STREAM ? 0 : keep_windows(ctx, ldx, g);   // (the 16-row kernels only)
    if (rows == 16 && wide) {
        // sixteen draws per pass
        if (nt) hipLaunchKernelGGL((blr_pass_mx_kernel<true, 4>), dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y,
                                   B, W, sg, slab, g.n_iter, rev, keep);
        else hipLaunchKernelGGL((blr_pass_mx_kernel<false, 4>), dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y,
                                B, W, sg, slab, g.n_iter, rev, keep);
    } else if (rows == 16) {
        // both contractions on v_mfma_f32_4x4x1, the tile by LDS-DMA
        unsigned long long* stamps = nullptr;
        if (ctx->blr_stamps && !ctx->capturing) {
            (void)stamp_buffer(ctx);
            stamps = (unsigned long long*)ctx->stamps;
            ctx->stamp_rows = g.n_blocks <= MAX_SLAB_ROWS ? g.n_blocks : 0;
            if (!ctx->stamp_rows) stamps = nullptr;
        }
        // windows of every workgroup / of the even ones (QSched): `blr_q_bias` per mille more for the even ones
        const int64_t n_tiles = (B + MT_ROWS - 1) / MT_ROWS;
        const int64_t w_all = (int64_t)g.n_blocks * PASS_WAVES, w_a = (int64_t)((g.n_blocks + 1) / 2) * PASS_WAVES;
        int extra = (int)((int64_t)g.n_iter * ctx->blr_q_bias + 500) / 1000;
        if (g.n_blocks < 2 || sweep != BSC_SWEEP_STREAM) extra = 0;
        int64_t rest = n_tiles - (int64_t)extra * w_a;
        if (rest < 0) { rest = n_tiles; extra = 0; }
        const int n_all = extra ? (int)((rest + w_all - 1) / w_all) : g.n_iter;
        const int n_a = n_all + extra;
#define BSC_PASS_Q(NT_, DBG_, PRIO_)                                                               \
    hipLaunchKernelGGL((blr_pass_q_kernel<NT_, DBG_, PRIO_>), dim3(g.n_blocks), dim3(PASS_BLOCK), 0, \
                       ctx->stream, X, ldx, y, B, W, sg, slab, n_all, n_a, rev, keep, stamps)
        if (ctx->blr_q_dbg == 1) BSC_PASS_Q(true, 1, 0);
        else if (ctx->blr_q_dbg == 2) BSC_PASS_Q(true, 2, 0);
        else if (ctx->blr_q_dbg == 3) BSC_PASS_Q(true, 3, 0);
        else if (nt && ctx->blr_q_prio == 1) BSC_PASS_Q(true, 0, 1);
        else if (nt && ctx->blr_q_prio == 2) BSC_PASS_Q(true, 0, 2);
        else if (nt) BSC_PASS_Q(true, 0, 0);
        else BSC_PASS_Q(false, 0, 0);
#undef BSC_PASS_Q
    } else if (rows == 8) {
        if (nt) launch_pass_rows<8, true>(ctx, X, ldx, y, B, D, W, sg, g, slab);
        else launch_pass_rows<8, false>(ctx, X, ldx, y, B, D, W, sg, g, slab);
    } else {
        if (nt) launch_pass_rows<4, true>(ctx, X, ldx, y, B, D, W, sg, g, slab);
        else launch_pass_rows<4, false>(ctx, X, ldx, y, B, D, W, sg, g, slab);
    }
}

int data_pass_impl(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                   const float* W, int32_t S, double* Q, double* G, int sweep) {
    int rc = check_pass_args(X, ldx, y, B, D, W, S, FIN_MAX_S);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(Q && G, "bsc_blr_data_pass: null output");
    BSC_REQUIRE(sweep >= 0 && sweep <= 2, "bsc_blr_data_pass: sweep=%d (0, 1 or 2)", sweep);
    const PassGrid g = blr_pass_grid(ctx, B, pass_rows(ctx, D, y));
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (size_t)2 * g.n_blocks * SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    float* slab = (float*)ws;
    ctx->slab_rows = 0;  // the slab is consumed here
    const dim3 rgrid((SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    const bool wide_ok = pass_rows(ctx, D, y) == 16 && ctx->blr_wide;
    for (int s0 = 0; s0 < S;) {
        // nine or more draws left: sixteen per pass (blr_pass_mx_kernel<., 4>), two slabs
        const bool wide = wide_ok && S - s0 > SG;
        const int cap = wide ? 2 * SG : SG;
        const int sg = (S - s0 < cap) ? (S - s0) : cap;
        launch_pass(ctx, X, ldx, y, B, (int)D, W + (int64_t)s0 * D, sg, g, slab, sweep, wide);
        BSC_LAUNCH_CHECK();
        hipLaunchKernelGGL(blr_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, slab,
                           g.n_blocks, (int)D, (int)S, s0, Q, G);
        BSC_LAUNCH_CHECK();
        if (sg > SG) {
            hipLaunchKernelGGL(blr_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream,
                               slab + (int64_t)g.n_blocks * SLAB_STRIDE, g.n_blocks, (int)D, (int)S,
                               s0 + SG, Q, G);
            BSC_LAUNCH_CHECK();
        }
        s0 += sg;
        if (sweep != BSC_SWEEP_STREAM) sweep = 3 - sweep;   // the next sample group walks back
    }
    return BSC_OK;
}

int data_pass_partial_impl(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B,
                           int32_t D, const float* W, int32_t S, int sweep) {
    int rc = check_pass_args(X, ldx, y, B, D, W, S, SG);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(sweep >= 0 && sweep <= 2, "bsc_blr_data_pass_partial: sweep=%d (0, 1 or 2)", sweep);
    const PassGrid g = blr_pass_grid(ctx, B, pass_rows(ctx, D, y));
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (size_t)2 * g.n_blocks * SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    launch_pass(ctx, X, ldx, y, B, (int)D, W, (int)S, g, (float*)ws, sweep);
    BSC_LAUNCH_CHECK();
    ctx->slab_rows = g.n_blocks;
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_blr_pass_count(bsc_ctx* ctx, const float* y, int32_t D, int32_t S, int32_t* count) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(count && S >= 1 && D >= 1, "bsc_blr_pass_count: bad arguments");
    const bool wide_ok = pass_rows(ctx, D, y) == 16 && ctx->blr_wide;
    int n = 0;
    for (int s0 = 0; s0 < S; ++n) {
        const int cap = (wide_ok && S - s0 > SG) ? 2 * SG : SG;
        s0 += (S - s0 < cap) ? (S - s0) : cap;
    }
    *count = n;
    return BSC_OK;
}

int bsc_blr_read_stamps(bsc_ctx* ctx, uint64_t* host_stamps, int32_t capacity_rows, int32_t* host_rows) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(host_stamps && host_rows && capacity_rows >= 0, "bsc_blr_read_stamps: bad arguments");
    BSC_HIP(hipStreamSynchronize(ctx->stream));
    const int n = ctx->stamps ? (ctx->stamp_rows < capacity_rows ? ctx->stamp_rows : capacity_rows) : 0;
    if (n > 0) BSC_HIP(hipMemcpy(host_stamps, ctx->stamps, (size_t)n * 64, hipMemcpyDeviceToHost));
    // the last stamped finish (option blr_finish_stamps) follows the pass's rows
    int nf = ctx->stamps ? ctx->fin_stamp_rows : 0;
    if (nf > capacity_rows - n) nf = capacity_rows - n;
    if (nf > 0)
        BSC_HIP(hipMemcpy(host_stamps + 8 * (size_t)n, (const char*)ctx->stamps + (size_t)MAX_SLAB_ROWS * 64, (size_t)nf * 64,
                          hipMemcpyDeviceToHost));
    *host_rows = n + nf;
    return BSC_OK;
}

int bsc_philox_normal(bsc_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t step,
                      int32_t n_samples, int32_t n_params, double* eps) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(eps && n_samples > 0 && n_params > 0, "bsc_philox_normal: bad arguments");
    const int n = n_samples * ((n_params + 3) / 4);
    hipLaunchKernelGGL(philox_normal_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                       seed, stream, step, n_samples, n_params, eps);
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

int bsc_blr_sample(bsc_ctx* ctx, const double* lam, int32_t D, int32_t S, uint64_t seed,
                   uint32_t step, double* eps, float* W, double* xi) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(lam && eps && W && xi && D > 0 && S > 0, "bsc_blr_sample: bad arguments");
    const int n = S * ((D + 3) / 4) + S;
    hipLaunchKernelGGL(blr_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                       lam, D, S, seed, step, eps, W, xi);
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

int bsc_blr_noise(bsc_ctx* ctx, int32_t D, int32_t S, uint64_t seed, uint32_t step0,
                  int32_t n_steps, double* eps) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(eps && D > 0 && S > 0 && n_steps > 0, "bsc_blr_noise: bad arguments");
    const int64_t n = (int64_t)(S * ((D + 3) / 4) + S) * n_steps;
    hipLaunchKernelGGL(blr_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, (int)D, (int)S, seed, step0, (int)n_steps, eps);
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

int bsc_blr_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B,
                      int32_t D, const float* W, int32_t S, double* Q, double* G) {
    BSC_CHECK_CTX(ctx);
    return data_pass_impl(ctx, X, ldx, y, B, D, W, S, Q, G, BSC_SWEEP_STREAM);
}

int bsc_blr_data_pass_sweep(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B,
                            int32_t D, const float* W, int32_t S, double* Q, double* G,
                            int32_t sweep) {
    BSC_CHECK_CTX(ctx);
    return data_pass_impl(ctx, X, ldx, y, B, D, W, S, Q, G, sweep);
}

int bsc_blr_data_pass_partial(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                              int64_t B, int32_t D, const float* W, int32_t S) {
    BSC_CHECK_CTX(ctx);
    return data_pass_partial_impl(ctx, X, ldx, y, B, D, W, S, BSC_SWEEP_STREAM);
}

int bsc_blr_data_pass_partial_sweep(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                                    int64_t B, int32_t D, const float* W, int32_t S,
                                    int32_t sweep) {
    BSC_CHECK_CTX(ctx);
    return data_pass_partial_impl(ctx, X, ldx, y, B, D, W, S, sweep);
}

int bsc_blr_elbo_grad(bsc_ctx* ctx, const double* lam, const double* eps, const float* W,
                      const double* xi, const double* Q, const double* G, int32_t D, int32_t S,
                      double batch_rows, double scale, double alpha0, double beta0, double* elbo,
                      double* grad) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(lam && eps && W && xi && Q && G && elbo && grad, "bsc_blr_elbo_grad: null pointer");
    BSC_REQUIRE(D > 0 && S >= 1 && S <= FIN_MAX_S, "bsc_blr_elbo_grad: D=%d S=%d (S<=%d)", D, S,
                FIN_MAX_S);
    BSC_REQUIRE(alpha0 > 0 && beta0 > 0, "bsc_blr_elbo_grad: alpha0, beta0 must be positive");
    hipLaunchKernelGGL(blr_elbo_grad_kernel, dim3(1), dim3(FIN_BLOCK), 0, ctx->stream, lam, eps, W,
                       xi, Q, G, (int)D, (int)S, batch_rows, scale, alpha0, beta0, elbo, grad);
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

namespace {
int fused_update_impl(bsc_ctx* ctx, const char* who, const double* stats, const double* lam_in, double* lam_out,
                      double* m1, double* m2, const double* eps, const float* W, const double* xi, int32_t D,
                      int32_t S, double c0, double c_xi, double s_q, double k_w, double beta, int64_t t, double lr,
                      double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                      double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next, double* elbo,
                      double* grad) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(lam_in && lam_out && m1 && m2 && eps && W && xi && elbo && grad, "%s: null pointer", who);
    BSC_REQUIRE(lam_in != lam_out, "%s: lam_in and lam_out must differ", who);
    BSC_REQUIRE(D > 0 && S >= 1 && S <= FIN_MAX_S, "%s: D=%d S=%d (S<=%d)", who, D, S, FIN_MAX_S);
    BSC_REQUIRE(t >= 1, "%s: the Adam step count starts at 1", who);
    // (the kernel draws the next step's noise itself where the caller has not: nothing is drawn here)
    const int rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, xi, eps_next, W_next, xi_next, D, S, seed,
                                   next_step, /*eps_next_ready=*/1);
    if (rc != BSC_OK) return rc;
    FusedArgs a;
    a.stats = stats;
    a.slab = nullptr;
    a.n_slab = 0;
    if (!stats) {
        BSC_REQUIRE(ctx->slab_rows > 0 && ctx->workspace,
                    "%s: stats is null and no bsc_blr_data_pass_partial slab is pending", who);
        BSC_REQUIRE(S <= SG && D <= GCOLS, "%s: slab input needs S<=8, D<=256", who);
        a.slab = (const float*)ctx->workspace;
        a.n_slab = ctx->slab_rows;
    }
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.xi = xi;
    a.eps_next = eps_next; a.W_next = W_next; a.xi_next = xi_next;
    a.eps_next_ready = eps_next_ready != 0;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.c0 = c0; a.c_xi = c_xi; a.s_q = s_q; a.k_w = k_w; a.beta = beta;
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    a.seed = seed;
    a.next_step = next_step;
    a.stamps = nullptr;
    const dim3 fgrid((D + 7) / 8 + 1);
    ctx->fin_stamp_rows = 0;
    if (ctx->blr_finish_stamps && !ctx->capturing && stamp_buffer(ctx)) {
        // behind the pass's rows: a pass stamped by blr_stamps in the same update keeps its own
        a.stamps = (unsigned long long*)ctx->stamps + 8 * (size_t)MAX_SLAB_ROWS;
        const int wgs = (int)fgrid.x < FIN_STAMP_WGS ? (int)fgrid.x : FIN_STAMP_WGS;
        ctx->fin_stamp_rows = wgs * (FIN_STAMPS / 8);
    }
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
#define BSC_FINISH(BLOCK_)                                                                                         \
    do {                                                                                                           \
        if (a.stamps) hipLaunchKernelGGL((blr_fused_update_kernel<BLOCK_, true>), fgrid, dim3(BLOCK_), 0, ctx->stream, a);  \
        else hipLaunchKernelGGL((blr_fused_update_kernel<BLOCK_, false>), fgrid, dim3(BLOCK_), 0, ctx->stream, a); \
    } while (0)
        if (ctx->blr_finish_block == 256) BSC_FINISH(256);
        else if (ctx->blr_finish_block == 512) BSC_FINISH(512);
        else BSC_FINISH(1024);
#undef BSC_FINISH
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}
}  // namespace

int bsc_blr_fused_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out,
                         double* m1, double* m2, const double* eps, const float* W,
                         const double* xi, int32_t D, int32_t S, double batch_rows, double scale,
                         double alpha0, double beta0, int64_t t, double lr, double beta1,
                         double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                         double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next,
                         double* elbo, double* grad) {
    BSC_REQUIRE(alpha0 > 0 && beta0 > 0, "bsc_blr_fused_update: bad hyper-parameters");
    // config 2 (oracle.svi.blr_log_joint) as a member of the family:
    //   scale [-B/2 (log 2 pi + xi) - e Q / 2] - D/2 (log 2 pi + xi) - e |w|^2 / 2 + alpha0 log beta0 - lnGamma(alpha0) - alpha0 xi - beta0 e
    const double half = 0.5 * (scale * batch_rows + (double)D);
    return fused_update_impl(ctx, "bsc_blr_fused_update", stats, lam_in, lam_out, m1, m2, eps, W, xi, D, S,
                             -half * BSC_LOG_2PI + alpha0 * log(beta0) - lgamma(alpha0), -half - alpha0, scale, 1.0, beta0,
                             t, lr, beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next,
                             xi_next, elbo, grad);
}

namespace {
// One update = the two launches bsc_blr_data_pass_partial_sweep + bsc_blr_fused_update[_general] (stats = NULL) make.
int pass_update_impl(bsc_ctx* ctx, const char* who, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                     int32_t sweep, const double* lam_in, double* lam_out, double* m1, double* m2, const double* eps,
                     const float* W, const double* xi, int32_t S, double c0, double c_xi, double s_q, double k_w,
                     double beta, int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                     uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next,
                     double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    int rc = check_pass_args(X, ldx, y, B, D, W, S, SG);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(sweep >= 0 && sweep <= 2, "%s: sweep=%d (0, 1 or 2)", who, sweep);
    rc = data_pass_partial_impl(ctx, X, ldx, y, B, D, W, S, sweep);
    if (rc != BSC_OK) return rc;
    return fused_update_impl(ctx, who, nullptr, lam_in, lam_out, m1, m2, eps, W, xi, D, S, c0, c_xi, s_q, k_w, beta, t,
                             lr, beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, xi_next,
                             elbo, grad);
}
}  // namespace

int bsc_blr_pass_update(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D, int32_t sweep,
                        const double* lam_in, double* lam_out, double* m1, double* m2, const double* eps, const float* W,
                        const double* xi, int32_t S, double batch_rows, double scale, double alpha0, double beta0,
                        int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                        uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next,
                        double* elbo, double* grad) {
    BSC_REQUIRE(alpha0 > 0 && beta0 > 0, "bsc_blr_pass_update: bad hyper-parameters");
    const double half = 0.5 * (scale * batch_rows + (double)D);       // (config 2 as a member of the family: bsc_blr_fused_update)
    return pass_update_impl(ctx, "bsc_blr_pass_update", X, ldx, y, B, D, sweep, lam_in, lam_out, m1, m2, eps, W, xi, S,
                            -half * BSC_LOG_2PI + alpha0 * log(beta0) - lgamma(alpha0), -half - alpha0, scale, 1.0, beta0, t, lr,
                            beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, xi_next, elbo, grad);
}

int bsc_blr_pass_update_general(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                                int32_t sweep, const double* lam_in, double* lam_out, double* m1, double* m2,
                                const double* eps, const float* W, const double* xi, int32_t S, double c0, double c_xi,
                                double s_q, double k_w, double beta, int64_t t, double lr, double beta1, double beta2,
                                double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                                int32_t eps_next_ready, float* W_next, double* xi_next, double* elbo, double* grad) {
    BSC_REQUIRE(s_q >= 0.0 && k_w >= 0.0, "bsc_blr_pass_update_general: s_q=%g k_w=%g must not be negative", s_q, k_w);
    return pass_update_impl(ctx, "bsc_blr_pass_update_general", X, ldx, y, B, D, sweep, lam_in, lam_out, m1, m2, eps, W, xi,
                            S, c0, c_xi, s_q, k_w, beta, t, lr, beta1, beta2, adam_eps, seed, next_step, eps_next,
                            eps_next_ready, W_next, xi_next, elbo, grad);
}

int bsc_blr_fused_update_general(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out,
                                 double* m1, double* m2, const double* eps, const float* W, const double* xi,
                                 int32_t D, int32_t S, double c0, double c_xi, double s_q, double k_w, double beta,
                                 int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                                 uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next,
                                 double* xi_next, double* elbo, double* grad) {
    BSC_REQUIRE(s_q >= 0.0 && k_w >= 0.0, "bsc_blr_fused_update_general: s_q=%g k_w=%g must not be negative", s_q, k_w);
    return fused_update_impl(ctx, "bsc_blr_fused_update_general", stats, lam_in, lam_out, m1, m2, eps, W, xi, D, S,
                             c0, c_xi, s_q, k_w, beta, t, lr, beta1, beta2, adam_eps, seed, next_step, eps_next,
                             eps_next_ready, W_next, xi_next, elbo, grad);
}

}  // extern "C"
