// The body of the predictive pass (csrc/bsc_predict.hip's header comment describes it), as a __device__ template over
// the likelihood family F -- a struct of csrc/bsc_families.h, which holds everything a family is: nothing here names one
// but the ordinal family, which keeps a branch of its own -- and compile-time flags, so that several translation units
// can instantiate it: OFFS = false is predict_kernel of
// csrc/bsc_predict.hip, unchanged; OFFS = true is predict_offset_kernel of csrc/bsc_predict_offset.hip, which adds a
// per-row offset o_n to l_ns = x_n . w_s before the link (logistic and Poisson families: log E[y_n] = x_n . w +
// log exposure_n).  GRP = true (always with OFFS) is predict_group_kernel of csrc/bsc_predict_group.hip: a per-draw,
// per-group intercept b_s[g_n] joins o_n, gathered from a table Bt [J + 1][ldb] by the row's group id (PredictGroups
// below).  With GRP off nothing of it is compiled: the shipped instantiations keep their code.  The host side at the end
// is the envelope of the entry points (predict_check_batch, predict_setup, predict_launch_chunks), shared by
// csrc/bsc_predict.hip, csrc/bsc_glm_nb.hip, csrc/bsc_glm_gamma.hip, csrc/bsc_glm_weibull.hip,
// csrc/bsc_glm_weibull_interval.hip, csrc/bsc_glm_beta.hip, csrc/bsc_glm_ordinal.hip and csrc/bsc_predict_group.hip.
// Header-only, internal linkage, like csrc/bsc_regress.h.
#pragma once

#include "bsc_families.h"

namespace {

constexpr int P_ORD_K = 8;                     // classes of the ordinal family at most
constexpr int P_BLOCK = 512;
constexpr int P_WAVES = P_BLOCK / BSC_WAVE;
constexpr int T_ROWS = 16;                     // rows per tile = the MFMA's N
constexpr int STRIP = 128;                     // columns per strip
constexpr int XS = STRIP + 2;                  // LDS row stride of a strip (floats)
constexpr int WCOLS = 256;                     // column capacity
constexpr int WS = WCOLS + 2;                  // LDS row stride of the draws
constexpr int LD_STRIP = STRIP * T_ROWS / (4 * BSC_WAVE);   // 16-byte loads per lane and strip: 8

typedef float p_f32x4 __attribute__((ext_vector_type(4)));

struct PredictArgs {
    const float* X;
    int64_t ldx;
    const float* y;          // may be null
    int64_t B;
    const float* W;
    const float* logvar;     // F::PER_DRAW: the family's scalar per draw (Gaussian: log s2; a scalar family: tau)
    float* mean;            // outputs, each may be null
    float* var;
    float* lpd;
    double* partial;         // [gridDim.x] block sums of lpd
    int D, S;
    int n_iter;              // tiles per wave
    int n_strips;            // strips per tile: 1 (D <= 128) or 2
    int kw;                  // columns per lane group and strip (even)
    int do_lp;               // y is set and lpd or lpd_sum is wanted
};

struct Strip {
    float4 x[LD_STRIP];
};

// Strip h of the tile from row0 on: lane -> (row 2 r + lane / 32, columns 128 h + 4 (lane % 32) ..).
__device__ __forceinline__ void load_strip(Strip& t, const PredictArgs& a, int64_t row0, int h, int lane) {
    auto xs = bsc_rows_rsrc(a.X, a.ldx, a.D, a.B, row0);
    const unsigned row_bytes = (unsigned)(a.ldx * 4);
    const int col = STRIP * h + 4 * (lane & 31);
    const int voff = (int)((unsigned)(lane >> 5) * row_bytes + 4u * (unsigned)col);
#pragma unroll
    for (int r = 0; r < LD_STRIP; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, voff, (int)(2u * r * row_bytes), 2);   // non-temporal
        float4 f = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                               __uint_as_float(v[3]));
        if (col >= a.D) f = make_float4(0.f, 0.f, 0.f, 0.f);   // padding, or the next row's bytes
        t.x[r] = f;
    }
}

__device__ __forceinline__ float load_y(const PredictArgs& a, int64_t row0, int i16) {
    auto ys = bsc_vec_rsrc(a.y, a.y ? a.B : 0, row0);
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ys, 4 * i16, 0, 0));
}

__device__ __forceinline__ float load_offset(const float* __restrict__ offset, int64_t B, int64_t row0, int i16) {
    auto os = bsc_vec_rsrc(offset, B, row0);
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(os, 4 * i16, 0, 0));
}

// GRP: the group ids of the rows, g [B] (int32; -1 = a group not seen in training), and the intercept draws
// Bt [J + 1][ldb] (float32, draws contiguous: Bt[j][s] = b_s[j], row J the unseen group's draws).
struct PredictGroups {
    const int32_t* g = nullptr;
    const float* Bt = nullptr;
    int J = 0;
    int ldb = 0;
};
constexpr int P_MAX_LDB = 8192;   // (J + 2) ldb 4 stays below 2^32 at J = BSC_GLM_GROUP_MAX_J

// The tile's sixteen ids, loaded like y; rows past B read id 0 (their results are never stored).
__device__ __forceinline__ int load_group(const int32_t* __restrict__ g, int64_t B, int64_t row0, int i16) {
    auto gs = bsc_vec_rsrc(g, B, row0);
    return (int)__builtin_amdgcn_raw_buffer_load_b32(gs, 4 * i16, 0, 0);
}

// The intercepts of lane (i16, kq): draws 16 c + 4 kq .. + 3 of the row's group, one 16-byte load per chunk through a
// descriptor of exactly (J + 1) ldb 4 bytes.  Id -1 is row J; every other id outside [0, J) goes to row J + 1, which
// is past the descriptor and reads zeros.  The whole offset is in the per-lane operand, the one the range check
// covers.  Columns from ldb on are the next row's bytes (or past the table: zeros): they are draws >= S, which `valid`
// masks by a select, and nothing is done to the loaded registers here -- a select at this point would make the
// compiler wait for the gather where it is issued.
template <int NC>
__device__ __forceinline__ void load_intercepts(p_f32x4 (&bt)[NC], const PredictGroups& gr, int id, int kq) {
    auto bs = __builtin_amdgcn_make_buffer_rsrc((void*)gr.Bt, 0, (unsigned)(gr.J + 1) * (unsigned)gr.ldb * 4u,
                                                0x00020000);
    unsigned row = id == -1 ? (unsigned)gr.J : (unsigned)id;
    row = row < (unsigned)gr.J + 1u ? row : (unsigned)gr.J + 1u;
    const int base = (int)(row * (unsigned)gr.ldb * 4u) + 16 * kq;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(bs, base + 64 * c, 0, 0);
        bt[c] = p_f32x4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
    }
}

// PREDICT_ORDINAL: what the family needs besides PredictArgs.  The draws are a.W = Z [S, ldz] with the weights in
// columns 0 .. D-1 and theta_0 = c_0, theta_j = log(c_j - c_{j-1}) behind them (4-byte aligned).
struct PredictOrdinal {
    float* prob = nullptr;   // [B, K], may be null
    int64_t ldz = 0;
    int K = 0;
};

// The two tables of the ordinal family, [draw][class] each, by thread (draw tid / 8, class tid % 8) of the 512: the
// cutpoints c_k (k < K - 1; +infinity from there on, so that sigmoid(c_k - l) = 1) as the float32 roundings of the
// float64 cumulative sum of the float32 theta, and log(-expm1(-g_k)) of the float32 gap g_k = c_k - c_{k-1} of an inner
// class (0 for the two end classes), made in float64 and rounded: csrc/bsc_glm_ordinal.hip's constants.
__device__ __forceinline__ void predict_ordinal_tables(float* ct, float* lt, const PredictArgs& a,
                                                       const PredictOrdinal& od, int tid) {
    const int s = tid >> 3, k = tid & 7, K = od.K;
    double c = 0.0;
    float lo = 0.f, hi = INFINITY;
    for (int j = 0; j < K - 1; ++j) {
        const float th = s < a.S ? a.W[(int64_t)s * od.ldz + a.D + j] : 0.0f;
        c = j == 0 ? (double)th : c + exp((double)th);
        if (j == k - 1) lo = (float)c;
        if (j == k) hi = (float)c;
    }
    const bool mid = k >= 1 && k <= K - 2;
    ct[tid] = hi;
    lt[tid] = mid ? (float)log(-expm1(-(double)(hi - lo))) : 0.0f;
}

// One (row, draw) of the ordinal family: pk[k] += P(y = k | l, c) for a valid draw, as the differences of the cumulative
// sigmoid(c_k - l) -- they telescope, so the K probabilities of a draw add up to 1 to rounding -- and the return value is
// log p(yq | l, c) in csrc/bsc_glm_ordinal.hip's form, -U sp(-b) - L sp(a) + log(-expm1(-g)), which does not cancel.
// cut: the draw's eight table entries; lg: the table's log(-expm1(-g)) at the row's class yq.
__device__ __forceinline__ float predict_link_ordinal(float l, const float (&cut)[P_ORD_K], float lg, int yq, bool U,
                                                      bool L, bool valid, float (&pk)[P_ORD_K]) {
    float prev = 0.0f, a_ = 0.0f, b_ = 0.0f;
#pragma unroll
    for (int k = 0; k < P_ORD_K; ++k) {
        const float x = cut[k] - l;
        const float e = expf(-fabsf(x));
        const float r = 1.0f / (1.0f + e);
        const float cum = x >= 0.0f ? r : e * r;
        pk[k] += valid ? cum - prev : 0.0f;
        prev = cum;
        b_ = yq == k ? x : b_;                 // flat selects: c_y - l and c_{y-1} - l
        a_ = yq == k + 1 ? x : a_;
    }
    const float xb = U ? -b_ : 0.0f, xa = L ? a_ : 0.0f;       // an end class: its missing side is evaluated at 0, unused
    const float eb = expf(-fabsf(xb)), ea = expf(-fabsf(xa));
    const float tb = 1.0f + eb, ta = 1.0f + ea;
    const float spb = fmaxf(xb, 0.0f) + (tb == 1.0f ? eb : logf(tb) * eb / (tb - 1.0f));
    const float spa = fmaxf(xa, 0.0f) + (ta == 1.0f ? ea : logf(ta) * ea / (ta - 1.0f));
    return lg - ((U ? spb : 0.0f) + (L ? spa : 0.0f));
}

// FULL: D == 256 (two strips, 32 columns per lane group, everything unrolled).
// The ordinal family (with OFFS; a null offset reads 0): `od` says where prob goes and how the draws are laid out;
// everything of it is behind `if constexpr`, and with another family nothing of it is compiled.
// OFFS: `offset` [B] (not null) is loaded like y and added to every draw's l of its row before the link.
// GRP (with OFFS; a null offset reads 0): the tile's ids are loaded with its y and offset, at `last` of the tile before;
// its intercepts are requested at the top of its first strip, ahead of that strip's LDS store, and land behind the
// tile's MFMAs.  Both loads are unconditional within their (wave-uniform) branch, so the X prefetch stays in flight.
// ITV (a family whose link takes upper ends, with OFFS): `upper` [B] (not null) is loaded like y and the offset; with the
// flag off nothing of it is compiled.
// F::PARAM (a scalar family with one constant per model): `par` goes to F::predict_slots, which puts what the link needs
// of it into the draws' slots; PredictArgs does not carry it.
template <class F, int NC, bool FULL, bool OFFS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void predict_body(PredictArgs a, const float* offset, PredictGroups gr = PredictGroups{},
                                             const float* upper = nullptr, PredictOrdinal od = PredictOrdinal{},
                                             float par = 0.f) {
    static_assert(!GRP || OFFS, "the grouped body adds its intercept next to the offset");
    static_assert(!ITV || (F::UPPER && OFFS && !GRP), "the upper end belongs to a family whose link takes one");
    constexpr bool ORD = F::PREDICT_ID == PREDICT_ORDINAL;
    static_assert(!ORD || (OFFS && !GRP && !ITV), "the ordinal family takes an offset and nothing else");
    constexpr int W_FLOATS = NC * 16 * WS;
    constexpr int X_FLOATS = P_WAVES * T_ROWS * XS;
    constexpr int GP_SLOTS = F::SCALAR ? 4 : 3;                           // F::predict_slots fills them, F::PER_DRAW
    constexpr int ORD_FLOATS = ORD ? 2 * P_ORD_K * P_MAX_S : 0;           // the cutpoints and log(-expm1(-g)), [draw][class]
    __shared__ __attribute__((aligned(16))) float lds[W_FLOATS + X_FLOATS + GP_SLOTS * P_MAX_S + ORD_FLOATS];
    __shared__ double red[P_WAVES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* wl = lds;                                    // draws [16 NC][WS], zero-padded
    float* xl = lds + W_FLOATS + wave * (T_ROWS * XS);  // this wave's strip [16][XS]
    float* gp = lds + W_FLOATS + X_FLOATS;              // the family's slots, [64] each
    [[maybe_unused]] float* ct = gp + GP_SLOTS * P_MAX_S;   // ORD: c_k, [64][8]
    [[maybe_unused]] float* lt = ct + P_ORD_K * P_MAX_S;    // ORD: log(-expm1(-g_k)), [64][8]
    const int S = a.S, D = a.D;

    for (int row = wave; row < NC * 16; row += P_WAVES)
        for (int col = lane; col < WS; col += BSC_WAVE)
            wl[row * WS + col] = (row < S && col < D) ? a.W[(int64_t)row * (ORD ? od.ldz : (int64_t)D) + col] : 0.f;
    if constexpr (ORD) predict_ordinal_tables(ct, lt, a, od, tid);
    if (tid < P_MAX_S) {
        const float lv = (F::PER_DRAW && tid < S) ? a.logvar[tid] : 0.f;
        if constexpr (F::PARAM) F::predict_slots(gp, tid, lv, par);
        else F::predict_slots(gp, tid, lv);
        if constexpr (F::PREDICT_ID == Gamma::PREDICT_ID) {   // (csrc/bsc_families.h says why this one slot is made here)
            const double al = (double)expf(lv);
            gp[3 * P_MAX_S + tid] = (float)(al * log(al) - bsc_lgamma_f64(al));
        }
    }
    __syncthreads();

    const int n_strips = FULL ? 2 : a.n_strips;
    const int kw = FULL ? 32 : a.kw;
    const int n_iter = a.n_iter;
    const int64_t B = a.B;
    const int64_t stride0 = (int64_t)gridDim.x * P_WAVES;
    const int64_t slot = (int64_t)blockIdx.x * P_WAVES + wave;
    auto row0_of = [=](int p) { return p < n_iter ? ((int64_t)p * stride0 + slot) * T_ROWS : B; };

    const float inv_S = 1.0f / (float)S;
    const float log_S = logf((float)S);
    double lsum = 0.0;

    p_f32x4 acc[NC][2];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c][0] = acc[c][1] = p_f32x4{0.f, 0.f, 0.f, 0.f};

    Strip t;
    load_strip(t, a, row0_of(0), 0, lane);
    float y_cur = load_y(a, row0_of(0), i16);
    float o_cur = 0.f;
    [[maybe_unused]] const int64_t o_rows = ((F::SCALAR || GRP || ORD) && !offset) ? 0 : a.B;   // null: no records, reads 0
    if constexpr (OFFS) o_cur = load_offset(offset, o_rows, row0_of(0), i16);
    [[maybe_unused]] float u_cur = 0.f;
    if constexpr (ITV) u_cur = load_offset(upper, a.B, row0_of(0), i16);
    [[maybe_unused]] int g_cur = 0;
    [[maybe_unused]] p_f32x4 bt[NC];
    if constexpr (GRP) {
#pragma unroll
        for (int c = 0; c < NC; ++c) bt[c] = p_f32x4{0.f, 0.f, 0.f, 0.f};
        g_cur = load_group(gr.g, a.B, row0_of(0), i16);
    }
    int p = 0, h = 0;
    while (p < n_iter) {
        if constexpr (GRP) {
            if (h == 0) load_intercepts<NC>(bt, gr, g_cur, kq);   // this tile's, ahead of its first LDS store
        }
        // the strip to LDS (row stride 130 floats: 8-byte aligned), its registers take the next strip
        {
            float* dst = xl + (lane >> 5) * XS + 4 * (lane & 31);
#pragma unroll
            for (int r = 0; r < LD_STRIP; ++r) {
                *reinterpret_cast<float2*>(dst + 2 * r * XS) = make_float2(t.x[r].x, t.x[r].y);
                *reinterpret_cast<float2*>(dst + 2 * r * XS + 2) = make_float2(t.x[r].z, t.x[r].w);
            }
        }
        int hn = h + 1, pn = p;
        if (hn == n_strips) {
            hn = 0;
            pn = p + 1;
        }
        load_strip(t, a, row0_of(pn), hn, lane);
        const bool last = hn == 0;
        float y_next = 0.f;
        if (last) y_next = load_y(a, row0_of(pn), i16);
        float o_next = 0.f;
        if constexpr (OFFS) {
            if (last) o_next = load_offset(offset, o_rows, row0_of(pn), i16);
        }
        if constexpr (GRP) {
            if (last) g_cur = load_group(gr.g, a.B, row0_of(pn), i16);   // consumed by the gather above, next iteration
        }
        [[maybe_unused]] float u_next = 0.f;
        if constexpr (ITV) {
            if (last) u_next = load_offset(upper, a.B, row0_of(pn), i16);
        }
        wave_lds_sync();

        const float* xr = xl + i16 * XS + kq * kw;
        const float* wr = wl + i16 * WS + h * STRIP + kq * kw;
        if (FULL) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float2 b = *reinterpret_cast<const float2*>(xr + 2 * j);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float2 w2 = *reinterpret_cast<const float2*>(wr + c * 16 * WS + 2 * j);
                    acc[c][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2.x, b.x, acc[c][0], 0, 0, 0);
                    acc[c][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2.y, b.y, acc[c][1], 0, 0, 0);
                }
            }
        } else {
            const int nj = kw >> 1;
            for (int j = 0; j < nj; ++j) {
                const float2 b = *reinterpret_cast<const float2*>(xr + 2 * j);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float2 w2 = *reinterpret_cast<const float2*>(wr + c * 16 * WS + 2 * j);
                    acc[c][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2.x, b.x, acc[c][0], 0, 0, 0);
                    acc[c][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2.y, b.y, acc[c][1], 0, 0, 0);
                }
            }
        }
        wave_lds_sync();   // the next iteration overwrites the strip

        if constexpr (ORD) {
            if (last) {
                // ---- the row's draws, as in the branch below; the label's bits ride in y_cur ----
                const int K = od.K;
                const int yi = (int)__float_as_uint(y_cur);
                const bool y_ok = (unsigned)yi < (unsigned)K;      // a label outside [0, K): the row scores 0
                const int yq = y_ok ? yi : 0;                       // what indexes the table is inside it
                const bool U = yq < K - 1, L = yq > 0;
                // The draws run in a LOOP, one after the other, with this lane's 4 NC linear predictors -- and then their
                // log p -- staged in the wave's strip buffer, which the MFMAs above are done with ([draw][lane]: no bank
                // conflicts, and only the lane itself reads what it wrote).  Unrolled, the sixteen draws' eight cumulative
                // terms apiece spill at NC = 4 and the code is ten exponentials per draw long.
                float* ls = xl + lane;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) ls[(4 * c + r) * BSC_WAVE] = acc[c][0][r] + acc[c][1][r] + o_cur;
                    acc[c][0] = acc[c][1] = p_f32x4{0.f, 0.f, 0.f, 0.f};
                }
                float pk[P_ORD_K];
#pragma unroll
                for (int k = 0; k < P_ORD_K; ++k) pk[k] = 0.f;
                float mx = -INFINITY;
#pragma unroll 1
                for (int i = 0; i < 4 * NC; ++i) {
                    const int d = 16 * (i >> 2) + 4 * kq + (i & 3);
                    const float4 c0 = *reinterpret_cast<const float4*>(ct + P_ORD_K * d);
                    const float4 c1 = *reinterpret_cast<const float4*>(ct + P_ORD_K * d + 4);
                    const float cut[P_ORD_K] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                    const bool valid = d < S;
                    const float lp_i = predict_link_ordinal(ls[i * BSC_WAVE], cut, lt[P_ORD_K * d + yq], yq, U, L, valid,
                                                            pk);
                    const float lpv = valid ? lp_i : -INFINITY;
                    ls[i * BSC_WAVE] = lpv;
                    mx = fmaxf(mx, lpv);
                }
#pragma unroll
                for (int k = 0; k < P_ORD_K; ++k) pk[k] = fold4_sum(pk[k]) * inv_S;
                float lpd = 0.f;
                if (a.do_lp) {
                    mx = fold4_max(mx);
                    const float ms = mx == -INFINITY ? 0.f : mx;   // every draw at -inf: lpd = -inf, not NaN
                    float se = 0.f;
#pragma unroll
                    for (int i = 0; i < 4 * NC; ++i) se += __expf(ls[i * BSC_WAVE] - ms);
                    se = fold4_sum(se);
                    lpd = y_ok ? ms + logf(se) - log_S : 0.f;
                }
                wave_lds_sync();   // the next strip overwrites the buffer
                const int64_t row = row0_of(p) + i16;
                if (kq == 0 && row < B) {     // lanes 0 .. 15: one row each
                    if (od.prob) {
#pragma unroll
                        for (int k = 0; k < P_ORD_K; ++k)
                            if (k < K) od.prob[row * K + k] = pk[k];
                    }
                    if (a.do_lp) {
                        if (a.lpd) a.lpd[row] = lpd;
                        lsum += (double)lpd;
                    }
                }
                y_cur = y_next;
                o_cur = o_next;
            }
        } else if (last) {
            // ---- the row's draws: register i = 4 c + reg of lane (i16, kq) is draw 16 c + 4 kq + reg ----
            const float yv = y_cur;
            float mu[4 * NC], lp[4 * NC];
            float s_mu = 0.f, s_v = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int d0 = 16 * c + 4 * kq;
                float4 lv4 = make_float4(0.f, 0.f, 0.f, 0.f), ev4 = lv4, iv4 = lv4;
                [[maybe_unused]] float4 lg4 = lv4;
                if (F::PER_DRAW) {
                    lv4 = *reinterpret_cast<const float4*>(gp + d0);
                    ev4 = *reinterpret_cast<const float4*>(gp + P_MAX_S + d0);
                    iv4 = *reinterpret_cast<const float4*>(gp + 2 * P_MAX_S + d0);
                }
                if constexpr (F::SCALAR) lg4 = *reinterpret_cast<const float4*>(gp + 3 * P_MAX_S + d0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float l = acc[c][0][r] + acc[c][1][r];
                    if constexpr (OFFS) l += o_cur;
                    if constexpr (GRP) l += bt[c][r];
                    const float lv = r == 0 ? lv4.x : r == 1 ? lv4.y : r == 2 ? lv4.z : lv4.w;
                    const float ev = r == 0 ? ev4.x : r == 1 ? ev4.y : r == 2 ? ev4.z : ev4.w;
                    const float iv = r == 0 ? iv4.x : r == 1 ? iv4.y : r == 2 ? iv4.z : iv4.w;
                    float m_i, v_i, lp_i, lg = 0.f;      // (u_cur and lg: 0 without ITV, without F::SCALAR; not read then)
                    if constexpr (F::SCALAR) lg = r == 0 ? lg4.x : r == 1 ? lg4.y : r == 2 ? lg4.z : lg4.w;
                    F::template predict_link<ITV>(l, yv, u_cur, lv, ev, iv, m_i, v_i, lp_i, lg);
                    const bool valid = d0 + r < S;
                    mu[4 * c + r] = valid ? m_i : 0.f;
                    lp[4 * c + r] = valid ? lp_i : -INFINITY;
                    s_mu += valid ? m_i : 0.f;
                    s_v += valid ? v_i : 0.f;
                }
                acc[c][0] = acc[c][1] = p_f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // two-pass moments: every lane of the row ends with the same mean, the squares are taken about it
            const float mean = fold4_sum(s_mu) / (float)S;
            float m2 = 0.f;
#pragma unroll
            for (int i = 0; i < 4 * NC; ++i) {
                const int d = 16 * (i >> 2) + 4 * kq + (i & 3);
                const float dv = mu[i] - mean;
                m2 = fmaf(d < S ? dv : 0.f, dv, m2);
            }
            m2 = fold4_sum(m2);
            s_v = fold4_sum(s_v);
            const float var = (s_v + m2) * inv_S;
            float lpd = 0.f;
            if (a.do_lp) {
                float mx = lp[0];
#pragma unroll
                for (int i = 1; i < 4 * NC; ++i) mx = fmaxf(mx, lp[i]);
                mx = fold4_max(mx);
                const float ms = mx == -INFINITY ? 0.f : mx;   // every draw at -inf: lpd = -inf, not NaN
                float se = 0.f;
#pragma unroll
                for (int i = 0; i < 4 * NC; ++i) se += __expf(lp[i] - ms);
                se = fold4_sum(se);
                lpd = ms + logf(se) - log_S;
                if (F::ROW_LGAMMA) lpd -= (float)bsc_lgamma_f64((double)yv + 1.0);   // once per row
            }
            const int64_t row = row0_of(p) + i16;
            if (kq == 0 && row < B) {     // lanes 0 .. 15: one row each, 64 contiguous bytes per output
                if (a.mean) a.mean[row] = mean;
                if (a.var) a.var[row] = var;
                if (a.do_lp) {
                    if (a.lpd) a.lpd[row] = lpd;
                    lsum += (double)lpd;
                }
            }
            y_cur = y_next;
            if constexpr (OFFS) o_cur = o_next;
            if constexpr (ITV) u_cur = u_next;
        }
        h = hn;
        p = pn;
    }

    if (a.partial) {   // fixed order: lanes (butterfly) -> waves -> block
        const double ws = wave_allsum_f64(lsum);
        if (lane == 0) red[wave] = ws;
        __syncthreads();
        if (tid == 0) {
            double tot = red[0];
#pragma unroll
            for (int k = 1; k < P_WAVES; ++k) tot += red[k];
            a.partial[blockIdx.x] = tot;
        }
    }
}

// ---- host side: the envelope of the predictive entry points, in two halves around the family's own checks ----------

#define PREDICT_UNSUPPORTED(cond, ...)                                    \
    do {                                                                  \
        if (!(cond)) return bsc_fail(BSC_ERR_UNSUPPORTED, __VA_ARGS__);   \
    } while (0)

inline int predict_check_batch(const char* who, const float* X, const float* y, int64_t B, const float* W,
                               const float* mean, const float* var, const float* lpd, const double* lpd_sum) {
    BSC_REQUIRE(B >= 0, "%s: B=%lld", who, (long long)B);
    BSC_REQUIRE((X || B == 0) && W, "%s: null pointer", who);
    BSC_REQUIRE(mean || var || lpd || lpd_sum, "%s: no output requested", who);
    BSC_REQUIRE(y || B == 0 || (!lpd && !lpd_sum), "%s: lpd and lpd_sum need y", who);
    return BSC_OK;
}

// What the entry points with a group table (csrc/bsc_predict_group.hip, csrc/bsc_predict_scalar_group.hip) ask of it;
// the alignment of the ids and of the family's other vectors stays with the caller, which names them.
inline int predict_check_groups(const char* who, const int32_t* groups, const float* Bt, int32_t J, int32_t ldb,
                                int32_t S) {
    PREDICT_UNSUPPORTED(groups && Bt, "%s: groups and Bt must not be null", who);
    PREDICT_UNSUPPORTED(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    PREDICT_UNSUPPORTED(ldb >= S && ldb % 4 == 0 && ldb <= P_MAX_LDB, "%s: ldb=%d must be >= S, %% 4 == 0 and <= %d",
                        who, ldb, P_MAX_LDB);
    PREDICT_UNSUPPORTED((((uintptr_t)Bt) & 15) == 0, "%s: Bt must be 16-byte aligned", who);
    return BSC_OK;
}

// The shapes the kernels take, the grid, the arguments and the workspace of lpd_sum's block partials.  *n_blocks = 0:
// an empty batch, lpd_sum is zeroed and there is nothing to launch.  w_mask: the alignment asked of the draws (3: the
// ordinal family, which reads them with 4-byte loads).
inline int predict_setup(bsc_ctx* ctx, const char* who, const float* X, int64_t ldx, const float* y, int64_t B,
                         int32_t D, const float* W, const float* logvar, int32_t S, float* mean, float* var, float* lpd,
                         double* lpd_sum, PredictArgs* args, int* n_blocks, unsigned w_mask = 15) {
    PREDICT_UNSUPPORTED(D > 0 && D <= WCOLS && D % 4 == 0, "%s: D=%d must be a multiple of 4 in [4,%d]", who, D, WCOLS);
    PREDICT_UNSUPPORTED(S >= 1 && S <= P_MAX_S, "%s: S=%d must be in [1,%d]", who, S, P_MAX_S);
    PREDICT_UNSUPPORTED(ldx >= D && ldx % 4 == 0 && ldx < ((int64_t)1 << 26),
                        "%s: ldx=%lld must be >= D, %% 4 == 0 and < 2^26", who, (long long)ldx);
    PREDICT_UNSUPPORTED(((uintptr_t)X & 15) == 0 && ((uintptr_t)W & w_mask) == 0,
                        w_mask == 15 ? "%s: X and W must be 16-byte aligned"
                                     : "%s: X must be 16-byte aligned and the draws 4-byte aligned",
                        who);
    *n_blocks = 0;
    if (B == 0) {
        if (lpd_sum) BSC_HIP(hipMemsetAsync(lpd_sum, 0, sizeof(double), ctx->stream));
        return BSC_OK;
    }
    // one workgroup per CU; every wave runs the same number of tiles
    const int64_t n_tiles = (B + T_ROWS - 1) / T_ROWS;
    const int64_t max_waves = (int64_t)P_WAVES * ctx->cu_count;
    const int64_t n_iter = (n_tiles + max_waves - 1) / max_waves;
    PREDICT_UNSUPPORTED(n_iter < ((int64_t)1 << 30), "%s: B=%lld is too large", who, (long long)B);
    const int64_t waves = (n_tiles + n_iter - 1) / n_iter;
    *n_blocks = (int)((waves + P_WAVES - 1) / P_WAVES);

    PredictArgs& a = *args;
    a.X = X; a.ldx = ldx; a.y = y; a.B = B; a.W = W; a.logvar = logvar;
    a.mean = mean; a.var = var; a.lpd = lpd; a.partial = nullptr;
    a.D = D; a.S = S;
    a.n_iter = (int)n_iter;
    a.n_strips = D > STRIP ? 2 : 1;
    a.kw = D > STRIP ? STRIP / 4 : ((D + 7) / 8) * 2;
    a.do_lp = (y && (lpd || lpd_sum)) ? 1 : 0;
    if (lpd_sum) {
        void* ws = nullptr;
        const int rc = bsc_workspace(ctx, (size_t)*n_blocks * sizeof(double), &ws);
        if (rc != BSC_OK) return rc;
        ctx->slab_rows = 0;   // pass partials that were pending in the workspace are gone
        a.partial = (double*)ws;
    }
    return BSC_OK;
}

// 16 draws per accumulator chunk: launch(NC) with NC = 1, 2 or 4 chunks as std::integral_constant (S in 33 .. 48 runs
// four, one of them empty).
template <class F>
void predict_launch_chunks(int S, F launch) {
    if (S <= 16) launch(std::integral_constant<int, 1>{});
    else if (S <= 32) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 4>{});
}

// (The entry point of the families with a per-draw scalar of their own -- csrc/bsc_glm_nb.hip, csrc/bsc_glm_gamma.hip,
// csrc/bsc_glm_weibull.hip, csrc/bsc_glm_weibull_interval.hip -- with its kernels: csrc/bsc_scalar_family.h.)

}  // namespace

// csrc/bsc_predict_offset.hip: the launch of predict_offset_kernel (family BSC_PREDICT_LOGISTIC or BSC_PREDICT_POISSON,
// offset not null), called from bsc_predict_pass_offset in csrc/bsc_predict.hip.  `predict_args` points to a
// PredictArgs: the struct has internal linkage in each translation unit (predict_kernel's mangled name carries it), so
// it crosses between the two as an untyped pointer.
void bsc_predict_offset_launch(bsc_ctx* ctx, int family, const void* predict_args, const float* offset, int n_blocks);
