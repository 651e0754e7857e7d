// Internal helpers shared by the kernels of libbayesic_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/bayesic_hip.h"
#include "bsc_special.h"   // bsc_digamma_f64, bsc_lgamma_f64 (and their conventions off x > 0)

constexpr int BSC_PROF_SLOTS = 3;
constexpr int BSC_EXCHANGE_SLOTS = 16;

struct bsc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    void* workspace = nullptr;   // partial-sum slabs; grown on demand
    size_t workspace_bytes = 0;
    int cu_count = 256;
    int blr_tile_rows = 16;      // 16: forward on the MFMA pipe when D == 256 (else 8-row VALU tiles); 8 | 4: VALU variants
    int blr_waves_per_simd = 0;  // tuning: cap resident waves per SIMD (0 = kernel's own limit)
    int fused_map_blocks_per_cu = 8;  // bsc_map_reduce, pure map: grid cap (256-thread blocks)
    int gram_dbg = 0;                 // deletion builds of gram256_bx_kernel (BSC_GRAM_DBG + BSC_PROFILING_BUILDS): WRONG results
    int rows_dbg = 0;                 // deletion builds of map_reduce_rows_f32_kernel (BSC_ROWS_DBG + BSC_PROFILING_BUILDS): WRONG results
    int rows_wg_per_cu = 64;          // map_reduce_rows_f32_kernel: workgroups per CU in the grid, eight of them resident (BSC_ROWS_WG; 0 = one step per wave)
    int skinny_nt_dbg = 0;            // deletion builds of gemm_skinny_nt_kernel (BSC_SKINNY_NT_DBG + BSC_PROFILING_BUILDS): WRONG results
    int skinny_nt_wg_per_cu = 1;      // gemm_skinny_nt_kernel: resident workgroups (4 waves, 64 KiB of rings each) per CU (BSC_SKINNY_NT_WG)
    int gemm_nt_c = 1;                // stream GEMM: results of 128 MiB and more leave by non-temporal stores (BSC_GEMM_NT_C=0 for A/B)
    int fused_map_flat = 1;           // pure maps with a contiguous float32 result: map_flat_f32_kernel (BSC_FUSED_MAP_FLAT=0: the round-1/2 kernels, for A/B)
    int gemm_fast = 1;                // GEMM: scalar-base loads for interior tiles (BSC_GEMM_FAST=0 turns them off)
    int gemm_skinny = 1;              // GEMM: the LDS-DMA kernels of csrc/bsc_skinny.hip for products with one tiny extent (BSC_GEMM_SKINNY=0 turns them off)
    int gemm_dma = 2;                 // GEMM: 2 = persistent stream-K on LDS-DMA operand tiles (gemm_f32_stream_kernel), 1 = one tile per workgroup with LDS-DMA operands (gemm_f32_dma_kernel), 0 = the register-staged kernel (BSC_GEMM_DMA)
    int lda_stream = 1;               // LDA statistic, K = 128: the persistent LDS-DMA kernel (BSC_LDA_STREAM=0: one column block per workgroup, register staging)
    int gemm_sym = 1;                 // GEMM: X^T X computes the tiles on and above the diagonal only (BSC_GEMM_SYM=0: all of them)
    int gemm_dbg = 0;                 // profiling only (BSC_GEMM_DBG): 1 = the stream kernel drops its whole-tile stores
    int fused_nt_store = 1;           // dense map: non-temporal stores of the result
    int bbvi_kernel = 1;         // bsc_logreg_bbvi_loglik (draws in LDS): 1 = X by LDS-DMA strips where eligible (S in 36..64, S % 4 == 0; X through VGPRs otherwise), 2 = X through VGPRs always
    int lda_dbg = 0;             // BSC_LDA_DBG: profiling-only deletion builds of the split-operand LDA kernel (1: no DMAs after the first two steps; 2: no arithmetic) -- wrong results
    int bbvi_dbg = 0;            // BSC_BBVI_DBG: profiling-only deletion builds of logreg_loglik_dma_kernel (wrong results)
    int csc_fast = 1;            // bsc_lda_sstats_csc: buffer-descriptor gathers (BSC_CSC_FAST=0 turns them off)
    int mfma_split = 0;          // 0: f32 MFMA (exact f32 products; the default and the dtype of every reported line); 2 / 3: f32 operands as sums of two / three bf16 terms on the bf16 MFMA, 3 / 6 products (csrc/bsc_bf16split.h; BSC_MFMA_SPLIT, bsc_set_mfma_split) where a kernel offers it
    int mog_nt = 0;              // bsc_mog_estep: 1 = non-temporal loads of X (BSC_MOG_NT).  Default 0: both half-waves read the same rows and the L2 keeps a row for the second one -- 1.01 x the algorithmic bytes instead of 1.19 x, same time (profiles/r03_pmc_kernels.txt)
    int wo_wg_per_cu = 2;        // bsc_weighted_outer: resident workgroups per CU the grid is sized for
    int fused_waves_per_cu = 16; // bsc_map_reduce: reduce splits target this many waves per CU
    int blr_q = 1;               // pinned: blr_pass_q_kernel (both contractions on v_mfma_f32_4x4x1, the tile by LDS-DMA) is the D = 256, S <= 8 pass
    int blr_q_dbg = 0;           // deletion builds of blr_pass_q_kernel (BSC_BLR_Q_DBG + BSC_PROFILING_BUILDS): WRONG results
    int blr_q_bias = 70;         // blr_pass_q_kernel, static schedule: per mille of further windows for the workgroups with an even blockIdx (QSched)
    int blr_q_prio = 1;          // blr_pass_q_kernel: s_setprio 1 from a tile's landing to the next tile's DMAs (1), or during the backward (2)
    int blr_stamps = 0;          // blr_pass_q_kernel: every workgroup leaves start / end s_memrealtime stamps and its XCD (bsc_blr_read_stamps)
    void* stamps = nullptr;      // 64 bytes per workgroup (words 0-3 used), allocated when blr_stamps is first used
    int stamp_rows = 0;          // workgroups of the last stamped launch
    int blr_finish_stamps = 0;   // blr_fused_update_kernel: thread 0 of every workgroup leaves one s_memrealtime stamp per stage
    int fin_stamp_rows = 0;      // 64-byte rows the last finish stamped (two per workgroup), behind the pass's in `stamps`
    int profiling_builds = 0;    // 1: the deletion builds (options marked dbg) may be selected -- WRONG results, timing only
    int blr_finish_block = 1024; // threads per workgroup of blr_fused_update_kernel (BSC_BLR_FINISH_BLOCK = 256 | 512 | 1024)
    int blr_nt_loads = 1;        // non-temporal loads of X (read once per pass): +9% measured
    int blr_keep = -1;           // windows a keeping sweep leaves in the Infinity Cache (BSC_BLR_KEEP; -1 = what fits 256 MiB)
    int blr_mx = 0;              // pinned: blr_pass_mx_kernel runs for S > 8 only (blr_wide)
    int blr_wide = 1;            // BSC_BLR_WIDE: S > 8 runs sixteen draws per pass (blr_pass_mx_kernel<., 4>); 0 = eight per pass
    int slab_rows = 0;  // block partials left in `workspace` by bsc_blr_data_pass_partial
    int capturing = 0;  // between bsc_capture_begin and bsc_capture_end: launches are recorded, not run
    // optional per-kernel timing of the dominant kernel (bsc_ctx_profile)
    int profile = 0;        // 0 = off, n = time every n-th launch of a dominant kernel
    // slot 0: the dominant kernel of an entry point; slot 1: the collective; slot 2: the finish kernel
    int profile_tick[BSC_PROF_SLOTS] = {0, 0, 0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events[BSC_PROF_SLOTS];  // recorded pairs
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;                    // reusable pairs
    // data-parallel exchange (csrc/bsc_comm.hip): an ncclComm_t, NULL = a world of one
    void* comm = nullptr;
    int comm_rank = 0;
    int comm_world = 1;
    // the overlapped exchange (bsc_allreduce_sum_begin / _end): collectives of finished pieces of a statistic run on a
    // second stream while the kernels of the next piece run on `stream`; one event pair per slot, created on first use
    hipStream_t comm_stream = nullptr;
    hipEvent_t xch_ready[BSC_EXCHANGE_SLOTS] = {};
    hipEvent_t xch_done[BSC_EXCHANGE_SLOTS] = {};
    int xch_pending[BSC_EXCHANGE_SLOTS] = {};
};

// Records an event pair around one launch when ctx->profile is on.
struct bsc_prof_scope {
    bsc_ctx* ctx;
    int slot;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    hipStream_t on;      // the stream the timed launch goes to (the context's own unless said otherwise)
    explicit bsc_prof_scope(bsc_ctx* c, int slot_ = 0, hipStream_t on_ = nullptr) : ctx(c), slot(slot_), on(on_ ? on_ : c->stream) {
        if (ctx->profile <= 0 || ctx->capturing) return;
        if ((ctx->profile_tick[slot]++ % ctx->profile) != 0) return;
        if (!ctx->prof_pool.empty()) {
            ev = ctx->prof_pool.back();
            ctx->prof_pool.pop_back();
        } else {
            (void)hipEventCreate(&ev.first);
            (void)hipEventCreate(&ev.second);
        }
        (void)hipEventRecord(ev.first, on);
    }
    ~bsc_prof_scope() {
        if (!ev.first) return;
        (void)hipEventRecord(ev.second, on);
        ctx->prof_events[slot].push_back(ev);
    }
};

// thread-local error message; returns `code` so callers can `return bsc_fail(...)`
int bsc_fail(int code, const char* fmt, ...);

// Make sure ctx->workspace holds at least `bytes`; may hipMalloc (synchronous).
int bsc_workspace(bsc_ctx* ctx, size_t bytes, void** out);

// csrc/bsc_skinny.hip: float32 products with one tiny extent that stream their large operand once
// through LDS-DMA.  Sets *handled = 1 when it took the product (then C is written / enqueued).
int bsc_gemm_skinny(bsc_ctx* ctx, int64_t M, int64_t N, int64_t K, const float* A, int64_t sa_m, int64_t sa_k,
                    const float* B, int64_t sb_k, int64_t sb_n, float* C, int64_t sc_m, int64_t sc_n, int* handled);

#define BSC_HIP(call)                                                            \
    do {                                                                         \
        hipError_t err__ = (call);                                               \
        if (err__ != hipSuccess)                                                 \
            return bsc_fail(BSC_ERR_HIP, "%s failed: %s (%s:%d)", #call,         \
                            hipGetErrorString(err__), __FILE__, __LINE__);       \
    } while (0)

#define BSC_REQUIRE(cond, ...)                                                   \
    do {                                                                         \
        if (!(cond)) return bsc_fail(BSC_ERR_INVALID, __VA_ARGS__);              \
    } while (0)

#define BSC_CHECK_CTX(ctx)                                                       \
    do {                                                                         \
        if ((ctx) == nullptr) return bsc_fail(BSC_ERR_INVALID, "null bsc_ctx");  \
        BSC_HIP(hipSetDevice((ctx)->device));                                    \
    } while (0)

#define BSC_LAUNCH_CHECK()                                                       \
    do {                                                                         \
        hipError_t err__ = hipGetLastError();                                    \
        if (err__ != hipSuccess)                                                 \
            return bsc_fail(BSC_ERR_HIP, "kernel launch failed: %s (%s:%d)",     \
                            hipGetErrorString(err__), __FILE__, __LINE__);       \
    } while (0)

// Kernel selection on the host: f receives the run-time flags (a count) as std::bool_constant (std::integral_constant)
// arguments, so a launch site names its kernel once with them as template arguments: kernel<A(), B()>.
template <class F>
void bsc_with_flags(F&& f) { f(); }
template <class F, class... Rest>
void bsc_with_flags(F&& f, bool flag, Rest... rest) {
    if (flag) bsc_with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else bsc_with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <int MAX, class F>
void bsc_with_count(int n, F&& f) {      // n in 1 .. MAX; a larger n runs MAX
    if constexpr (MAX > 1) {
        if (n < MAX) return bsc_with_count<MAX - 1>(n, f);
    }
    f(std::integral_constant<int, MAX>{});
}

constexpr int BSC_WAVE = 64;

// ---- wave-level helpers ---------------------------------------------------

// DPP controls (cdna4 ISA): quad_perm encodes the source lane of each quad lane.
constexpr int DPP_QUAD_XOR1 = 0xB1;  // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;  // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_ROR4 = 0x124;
constexpr int DPP_ROW_ROR8 = 0x128;

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// Sum over the 16 lanes of a DPP row, result in every lane of the row.
// Rotation direction does not matter: each stage is applied to a value that is
// already periodic with the stage's period.
__device__ __forceinline__ float row16_allsum(float v) {
    v += dpp_f32<DPP_QUAD_XOR1>(v);
    v += dpp_f32<DPP_QUAD_XOR2>(v);
    v += dpp_f32<DPP_ROW_ROR4>(v);
    v += dpp_f32<DPP_ROW_ROR8>(v);
    return v;
}

// Full 64-lane sum, result in every lane.
__device__ __forceinline__ float wave_allsum(float v) {
    v = row16_allsum(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}


// FOUR 64-lane float64 sums at once, without the LDS crossbar: the 16 lanes of DPP row q end with the sum of a_q over
// the wave.  v_permlane32_swap / v_permlane16_swap halve the lanes a value occupies while two values share a register
// pair (lanes 0..31 fold a0 resp. a1 over (l, l + 32), lanes 32..63 a2 resp. a3; then rows 0..3 fold (l, l + 16)),
// the last four steps are DPP rotations inside a row: 21 vector instructions for four sums, where four butterflies
// of __shfl_xor are 48 ds_bpermute_b32 in chains of six LDS round trips.  Fixed order: reproducible.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ double swap_add32_f64(double a, double b) {
    auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ double swap_add16_f64(double a, double b) {
    auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// One 64-lane float64 sum, result in every lane: DPP inside the rows, then the rows by the two swaps (a value swapped
// with itself: rows 0 / 1 and 2 / 3 exchange, then the halves) -- 22 vector instructions and no LDS round trip where
// six steps of __shfl_xor were twelve ds_bpermute_b32 in a dependent chain.
__device__ __forceinline__ double wave_allsum_f64(double v) {
    v += dpp_f64<DPP_QUAD_XOR1>(v);
    v += dpp_f64<DPP_QUAD_XOR2>(v);
    v += dpp_f64<DPP_ROW_ROR4>(v);
    v += dpp_f64<DPP_ROW_ROR8>(v);
    v = swap_add16_f64(v, v);
    return swap_add32_f64(v, v);
}
__device__ __forceinline__ double wave_allsum4_f64(double a0, double a1, double a2, double a3) {
    double t = swap_add16_f64(swap_add32_f64(a0, a2), swap_add32_f64(a1, a3));
    t += dpp_f64<DPP_QUAD_XOR1>(t);
    t += dpp_f64<DPP_QUAD_XOR2>(t);
    t += dpp_f64<DPP_ROW_ROR4>(t);
    t += dpp_f64<DPP_ROW_ROR8>(t);
    return t;
}

// Orders this wave's LDS writes before its later LDS reads of other lanes' data
// (wave-private LDS regions, no workgroup barrier).  LDS operations of one wave
// execute in order; this only stops the compiler from moving them.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- LDS-DMA helpers (csrc/bsc_bbvi.hip, csrc/bsc_skinny.hip) -------------------------------
typedef __attribute__((address_space(3))) void* bsc_lds_ptr;

// s_waitcnt immediate (gfx9 layout) that waits for vmcnt <= n only: vmcnt = [3:0] and [15:14],
// expcnt [6:4] and lgkmcnt [11:8] left at "no wait"
constexpr int bsc_vmcnt_only(int n) { return (n & 0xF) | ((n >> 4) << 14) | (0x7 << 4) | (0xF << 8); }
constexpr int BSC_LGKMCNT0 = 0xC07F;   // lgkmcnt(0) alone

// A descriptor over the rows of a row-major matrix from `row0` on (`rows` in all, `ld` floats
// apart, `width` floats wide): everything past the last row reads as zero.
__device__ __forceinline__ auto bsc_rows_rsrc(const float* X, int64_t ld, int width, int64_t rows, int64_t row0) {
    const int64_t rem = rows - row0;
    uint64_t xb = 0;
    if (rem > 0) xb = ((uint64_t)(rem - 1) * (uint64_t)ld + (uint64_t)width) * 4u;
    const unsigned rec = xb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)xb;
    return __builtin_amdgcn_make_buffer_rsrc((void*)(X + (rem > 0 ? row0 : 0) * ld), 0, rec, 0x00020000);
}
typedef decltype(bsc_rows_rsrc(nullptr, 0, 0, 0, 0)) bsc_rsrc_t;
// ... over a vector of 4-byte elements (one per row) from element `row0` on
__device__ __forceinline__ auto bsc_vec_rsrc(const void* base, int64_t n, int64_t row0) {
    const int64_t rem = n - row0;
    const uint64_t b = rem > 0 ? (uint64_t)rem * 4u : 0;
    const unsigned rec = b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)b;
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + (rem > 0 ? row0 : 0) * 4), 0, rec, 0x00020000);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Reads of DMA'd bytes are inline asm: the compiler cannot tell the slots of a ring apart and would wait for
// vmcnt(0) at every ds_read it can see next to a DMA in flight.  Valid after the next lgkmcnt(0), placed by hand.
#define BSC_LDS_B128(DST, ADDR, OFF) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF) : "memory")
#define BSC_LDS_B32(DST, ADDR, OFF) \
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF) : "memory")

// A wave's ring of 1-KiB slots for 16-row tiles of a row-major f32 matrix that arrive by LDS-DMA in WHOLE 128-byte
// lines (csrc/bsc_bbvi.hip's two DMA kernels, gemm_skinny_nt_kernel).  Piece s = 2 c + sp of a tile is rows
// 8 sp .. + 7 x columns 32 c .. + 31 (8 x 128 bytes; pieces shaped like one strip of MFMA operands, 16 rows x 64
// bytes, read 23 % slower -- tools/ab_skinny_nt.py); lane l of the DMA = (row a = l >> 3, 16-byte position p = l & 7).
// The 16-byte chunks of a row are XOR-permuted -- on the GLOBAL side, the fill stays lane-linear: the chunk fetched
// into position p of row a is p ^ f, f = (a >> 1) | (sp << 2) (voff0 for sp = 0, voff1 for sp = 1).  That makes the
// operand read of strip j = 2 c + t (the 16 columns of k-group j: lane (i16, kq) <- row i16, chunk kq + 4 t of column
// block c) ONE ds_read_b128 free of bank conflicts in each of the instruction's four 16-lane groups: at addr0 (t = 0)
// or addr1 = addr0 ^ 64 (t = 1), plus the offset of the slot that holds the block's piece sp = 0; piece sp = 1 is in
// the slot behind it.  voff and addr must agree bit for bit, which is why they live together.  Which slot a piece
// goes to, and the constant offsets of the reads, stay with the caller.  The constructor's i16 and kq MUST be
// lane & 15 and lane >> 4; they come in as the kernels hold them because, derived from `lane` in here, the addresses
// fold to other instructions and the kernels' set-up code moves.
struct bsc_line_ring {
    char* base;            // the wave's first slot
    int row_bytes;         // distance of the matrix's rows
    int voff0, voff1;      // the DMA's side, per lane: piece parity sp = 0, 1
    unsigned addr0, addr1; // the reader's side, per lane: strip parity t = 0, 1
    __device__ __forceinline__ bsc_line_ring(char* wave_base, int lane, int i16, int kq, int row_bytes_)
        : base(wave_base), row_bytes(row_bytes_) {
        const int ra = lane >> 3, rp = lane & 7;
        voff0 = ra * row_bytes + 16 * (rp ^ (ra >> 1));
        voff1 = ra * row_bytes + 16 * (rp ^ ((ra >> 1) | 4));
        const int sp = i16 >> 3, ar = i16 & 7;
        addr0 = (unsigned)(uintptr_t)(bsc_lds_ptr)base + 1024u * sp + 128u * ar + 16u * (kq ^ ((ar >> 1) | (sp << 2)));
        addr1 = addr0 ^ 64u;
    }
    __device__ __forceinline__ void dma(bsc_rsrc_t rs, int piece, int slot) const {     // nt: the matrix is read once
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (bsc_lds_ptr)(base + slot * 1024), 16, (piece & 1) ? voff1 : voff0,
                                                 (piece & 1) * 8 * row_bytes + 128 * (piece >> 1), 0, 2);
    }
};

__device__ __forceinline__ float readlane_f32(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
