"""The row passes at the LEADING DIMENSIONS their entry points admit.  Every data pass takes its matrix as (pointer, ld) and
turns ld into 32-bit arithmetic on the device: per-lane byte offsets row * (int)(ld * 4), buffer descriptors whose record
count is clamped to 0xFFFFFFFF once the remaining span passes 4 GiB, offsets r * row_bytes that pass 2^31 inside one
16-row tile.  Every other GPU test reads its rows at ld = D plus a few elements; here the rows lie up to 2^26 - 4 floats
apart inside ONE module-wide float32 buffer of 23 * (2^26 - 4) + 256 floats (5.75 GiB; `wide`), NaN everywhere except
the rows of the running case, so that a lane that reads another row's neighbourhood poisons the result instead of
faulting: the buffer covers the whole span the call's arguments describe, above the gates too.

Every below-gate case asserts (a) the float64 comparison of the entry point's dense test at that test's tolerance,
unchanged, and (b) BIT equality with the same entry point on a compact copy (ld = width) of the same rows in the same
context -- the partition of each of these passes depends on the row count, never on ld.  Each case prints its worst
error / bound (run with -s).  Above a BSC_REQUIRE / unsupported gate the call must raise BayesicHipError with the
documented message and leave the NaN-prefilled outputs untouched; a declining gate must take the general route and be right.

Tolerances, by the test they are taken from:
  bsc_blr_data_pass            test_view_routes_gpu.test_blr_data_pass_refuses (Q 3e-6 (q + 0.1 sum size^2); G 2e-5 scale + 3e-7 size)
  bsc_glm_data_pass            test_glm_gpu._check_pass (ell 2e-5 * sum(|y l| + A + 1); G rtol 1e-4, atol 1e-4 max|G|)
  bsc_softmax_data_pass        test_softmax_regression_gpu._assert_pass
  bsc_predict_pass             test_predict_gpu._check (_predict_ref.bounds)
  bsc_softmax_predict_pass     test_regression_multi_tile_gpu.test_softmax_predict_pass (_softmax_ref.predict_bounds)
  bsc_logreg_bbvi_loglik       test_bbvi_gpu.test_loglik_matches_oracle (2e-5 * sum(|l| + 1)), also on split operands
  bsc_weighted_outer           test_wouter_gpu (2e-5 * sum |R| |X| |Y|)
  bsc_mog_estep                test_view_routes_gpu.test_mog_estep (3e-5 * scale; lse rtol 3e-6, atol 1e-4); split operands:
                               test_mfma_split_gpu.test_mog_estep_on_split_operands (2e-5 * scale; lse rtol 2e-6, atol 1e-4)
  bsc_gemm_softmax_rows        test_softmax_gpu (R rtol 2e-5, atol 2e-6; lse 1e-5 and cross 2e-5 of max|logits| + 1)
  bsc_gemm_softmax_stats       test_softmax_stats_gpu (stats and column sums 3e-6 sum |R| |A| + 1e-6; lse_sum rtol 2e-6; the spare
                               column of stats stays NaN) and test_view_routes_gpu.test_gemm_softmax_refuses (R rtol 2e-5, atol 2e-6)
  Gram / skinny (S cases)      test_mfma_split_gpu.test_gram_statistic_on_split_operands (2e-5 |x_d| |x_e|);
                               test_view_routes_gpu.test_skinny (1e-5 |A| @ |B|)

One row per gate: the check, the case ids on either side, the kernel each side runs (profiles/span_routes_kernel_stats.csv).
Tile heights: 8 rows (VALU regression kernels), 16 rows (MFMA regression, predictive, BBVI), 32 rows (mixture, row softmax,
Gram), 64 rows (weighted outer).  "tile31": a byte offset >= 2^31 inside one tile; "total32": a span >= 2^32.

  bsc_regress.h check_regress_args: ldx < 2^26      below (24 rows, ld 2^26 - 4; total32, tile31 in the 16-row kernels):
      test_below_gate[blr-valu-D64] blr_pass_kernel<false, 8>; [blr-q-D256] blr_pass_q_kernel; [blr-mx-S16] blr_pass_mx_kernel;
      [blr-rows8-D256] blr_pass_kernel<true, 8> (option blr_tile_rows = 8); [glm-valu-D64] glm_pass_kernel;
      [glm-mfma-D256] glm_pass_mfma_kernel; [softmax-K5-D256] softmax_pass_kernel
      [blr-q-B1100-ld2^20]: 1100 rows 4 MiB apart -- descriptors clamped for the first tiles, unclamped for the last
                                                    above (20 rows, ld 2^26): test_refused[blr], [glm], [softmax]: "ldx=.. must be >= D"
  bsc_predict_pass.h: ldx < 2^26                    below: [predict-logistic-D256] predict_kernel; [softmax-predict-K3] softmax_predict_kernel
                                                    above: test_refused[predict], [softmax-predict]
  bsc_bbvi.hip bsc_logreg_bbvi_loglik: ldx < 2^26   below: [bbvi-dma-S64] logreg_loglik_dma_kernel; [bbvi-xreg-S8] logreg_loglik_xreg_kernel<., 1>;
      [bbvi-xreg-S64] the same kernel <., 4> (option bbvi_kernel = 2); [bbvi-bx-S64] logreg_loglik_dma_bx_kernel (mfma_split = 2)
                                                    above: test_refused[bbvi]: "bad ldx="
  bsc_wouter.hip: max(ldr, ldx, ldy) < 2^22         below (300 rows, ld 2^22 - 4, R | X | Y side by side in the same rows; total32):
      [wouter-sym] weighted_outer_kernel<2, 5>, Y == X; [wouter-xy] <1, 8>, Y != X    above: test_refused[wouter]: "below 2^22"
  bsc_mog.hip bsc_mog_estep: ldx < 2^25             below (40 rows, ld 2^25 - 4; row 31 at byte 4.16e9 < 2^32; tile31, total32):
      [mog-D16] mog_estep_kernel<true, false>; [mog-D5] mog_estep_kernel<false, true>; [mog-bx-D16] mog_estep_bx_kernel
                                                    above (ld 2^25): test_refused[mog]: "bad ldx="
  bsc_rowsoftmax.hip: lda < 2^25                    below: [gsr-K16], [gsr-K40], [gsr-K64] gemm_softmax_rows_kernel<8 / 20 / 32>;
      [gss-K24], [gss-K24-bias] gemm_softmax_stats_kernel                       above: test_refused[gsr], [gss]: ": lda="
      The limit was 2^26 in both files until this test: at ld = 2^26 - 4 the lane offset (lane & 31) * (int)(ld * 4) of rows
      17..31 wraps past 2^32 and lands inside the clamped descriptor, in another row's neighbourhood.
  device_backend.evaluate_softmax_rows: sxm < 2^25  test_softmax_of_a_product_on_a_far_view[below]: one bsc_gemm_softmax_rows;
                                                    [above]: the product and bsc_softmax_rows, and right
  bsc_gram.hip bsc_gram_split: ldx < 2^25           S cases (4100 rows, ld 327 680; total32): test_below_gate[gram-D64] gram_bx_kernel<2>,
      [gram-D256] gram256_bx_kernel.  NOT crossed: the route needs >= 4096 rows, 512 GiB at that stride
  bsc_skinny.hip small_span (ld < 2^26)             S cases: [skinny-nt] gemm_skinny_nt_kernel<2, 16>, [skinny-nt-swapped] <1, 4> (4100 rows, ld 327 680);
      [skinny-tn] gemm_skinny_tn_kernel (K = 16 384, sb_k = 81 920).  The ld < 2^26 limit of the NT routes stays uncrossed: they
      need >= 4096 rows (1 TiB at that stride); for TN the s * 15 + K gate binds first (test_view_routes_gpu.test_span_gates)

  the same ldx < 2^26 check in the weighted, grouped and learned-scalar passes (runners and tolerances: tests/_span_borrowed.py)
      below: [glm-obs-mfma-D256] glm_obs_pass_mfma_kernel, [glm-obs-valu-D64] glm_obs_pass_kernel (bsc_glm_data_pass_obs);
      [glm-groups-D256] glm_group_pass_mfma_kernel; [glm-nb-D256] scalar_pass_mfma_kernel<2> (the learned-scalar family's
      kernel set, bsc_glm_nb_data_pass); [weibull-interval-D256] scalar_upper_pass_mfma_kernel<4>; [ordinal-ldx]
      glm_ordinal_pass_mfma_kernel; [predict-offset-D256] predict_offset_kernel; [predict-groups-D256] predict_group_kernel
                                                    above: test_refused[glm-obs], [glm-groups], [glm-nb], [weibull-interval],
                                                    [ordinal-ldx], [predict-offset], [predict-groups]
  bsc_glm_ordinal.hip: ldz < 2^26                   below: [ordinal-ldz] glm_ordinal_pass_kernel<false> (24 draws 2^26 - 4 floats apart, X compact, D = 252)
                                                    above: test_refused[ordinal-ldz]: "ldz=.. must be >= D + K - 1 and < 2^26"
  bsc_lda.hip lda_sstats_impl, the stream kernel's three inequalities, one at a time (70 documents, V = 1028, K = 128):
      (31 ldc + VT) * 4 < 2^31                      below: [lda-C-below] lda_sstats_stream_kernel; above: test_declined..[lda-C-above] lda_sstats_kernel
      (31 ldth + K) * 4 < 2^31                      [lda-Th-below] / [lda-Th-above] likewise
      (K ldb + V) * 4 < 2^32                        [lda-Bt-below] / [lda-Bt-above] likewise
      the same inequalities in front of the split-operand kernels (option mfma_split): [lda-Bt-below-bx2] lda_sstats_bx2_kernel,
      [lda-C-below-bx2-bound] lda_sstats_bx2_bound_kernel, [lda-Th-below-bx3-bound] lda_sstats_bx3_bound_kernel

Kernels of tests/test_kernel_resources.py that take a stride and are NOT in the trace of this file, and why: the gemm_f32_*
kernels other than the general one (their span gates, dma_ok's lane offsets, are crossed by test_view_routes_gpu.test_span_gates;
the stream and LDS-DMA kernels decline every operand of this file by those gates); lda_sstats_csc_kernel (Theta through ldth
with 64-bit row addresses and no gate on it, the counts are sparse: not one of the row passes); the map / reduce kernels
of bsc_fused.hip (general strides per axis, 64-bit, no leading-dimension limit documented).  The Gram and skinny NT gates
themselves need >= 4096 rows at the limit's stride, 512 GiB and 1 TiB, beyond the 8 GiB cap.

First device run (MI355X), the worst error / bound per entry point over the cases of this file: bsc_blr_data_pass 0.016;
bsc_glm_data_pass 0.0016; bsc_softmax_data_pass 0.0017; bsc_predict_pass 0.014; bsc_softmax_predict_pass 0.0008;
bsc_logreg_bbvi_loglik 0.0038 (0.024 on split operands); bsc_weighted_outer 0.0021; bsc_mog_estep 0.04 (lse; 0.077 on split
operands); bsc_gemm_softmax_rows 0.20; bsc_gemm_softmax_stats 0.25; Gram 0.16; skinny NT 0.027, TN 0.0003; bsc_glm_data_pass_obs
0.003 and _groups 0.002 (both G); bsc_glm_nb_data_pass 0.014 (T); bsc_glm_weibull_data_pass_interval 0.0035;
bsc_glm_ordinal_data_pass 0.0039 (ldx), 0.0058 (ldz); bsc_predict_pass_offset 0.007; bsc_predict_pass_groups 0.004;
bsc_lda_sstats 0.012 (0.16 on two bf16 terms, 0.014 on three; the words' term 0.013).  Every below-gate case was
bit-identical to its compact run.  The module takes 3 s after collection (67 cases, the 5.75 GiB fill included) beside
16 s for test_view_routes_gpu.py's 912.
Against the library as it was before the limit of the 32-row kernels was lowered (24 rows, ld = 2^26 - 4) all eight cases of
bsc_mog_estep, bsc_gemm_softmax_rows and bsc_gemm_softmax_stats FAILED: rows 17..23 read NaN (7 of 24 lse values, every statistic).
"""
import contextlib
import math

import numpy as np
import numpy.testing as npt
import pytest

import _span_borrowed as borrowed

F32, F64 = np.float32, np.float64
LD26, LD25, LD22 = (1 << 26) - 4, (1 << 25) - 4, (1 << 22) - 4
WIDE_FLOATS = 23 * LD26 + 256
CAP_BYTES = 8 * (1 << 30)


def case(id, entry, rows, width, ld, limit, tile, claims=("total32",), options=None, ragged=True, **params):
    """limit: the first leading dimension the gate refuses; tile: the rows of one tile of the kernel that runs; ragged:
    whether the last tile is a partial one (24 rows are three FULL tiles of an 8-row kernel, and the row counts of the
    TN contraction and of Beta are what the issue and K set)."""
    return dict(id=id, entry=entry, rows=rows, width=width, ld=ld, limit=limit, tile=tile, claims=claims,
                options=options or {}, ragged=ragged, **params)


def _lda_case(which, side, tag="", options=None, bound=False):
    first = borrowed.lda_first_refused(which)
    ld = (first - 1) // 4 * 4 if side == "below" else (first + 3) // 4 * 4
    rows, width = dict(C=(borrowed.LDA_DOCS, borrowed.LDA_V), Th=(borrowed.LDA_DOCS, borrowed.LDA_K),
                       Bt=(borrowed.LDA_K, borrowed.LDA_V))[which]
    # Beta's inequality is on its whole span, K ldb + V floats: just below 2^32 bytes, so nothing past it is claimed
    return case("lda-%s-%s%s" % (which, side, tag), "lda", rows, width, ld, first, 32, () if which == "Bt" else ("total32",),
                options, ragged=which != "Bt", spread=which, bound=bound)


L16 = ("total32", "tile31")
BELOW = [
    # ---- L cases: 24 rows at 2^26 - 4 ----------------------------------------------------------------------------
    case("blr-valu-D64", "blr", 24, 64, LD26, 1 << 26, 8, ragged=False, D=64, S=8),
    case("blr-q-D256", "blr", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8),
    case("blr-mx-S16", "blr", 24, 256, LD26, 1 << 26, 16, L16, dict(blr_wide=1), D=256, S=16),
    case("blr-rows8-D256", "blr", 24, 256, LD26, 1 << 26, 8, options=dict(blr_tile_rows=8), ragged=False, D=256, S=8),
    case("blr-q-B1100-ld2^20", "blr", 1100, 256, 1 << 20, 1 << 26, 16, D=256, S=8),
    case("glm-valu-D64", "glm", 24, 64, LD26, 1 << 26, 8, ragged=False, D=64, S=8, link="logistic"),
    case("glm-mfma-D256", "glm", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=9, link="poisson"),
    case("softmax-K5-D256", "softmax", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=4, K=5),
    case("predict-logistic-D256", "predict", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=17, family="logistic"),
    case("softmax-predict-K3", "softmax_predict", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=7, K=3),
    case("bbvi-dma-S64", "bbvi", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=64),
    case("bbvi-xreg-S8", "bbvi", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8),
    case("bbvi-xreg-S64", "bbvi", 24, 256, LD26, 1 << 26, 16, L16, dict(bbvi_kernel=2), D=256, S=64),
    case("bbvi-bx-S64", "bbvi", 24, 256, LD26, 1 << 26, 16, L16, dict(mfma_split=2), D=256, S=64),
    # ---- 300 rows at 2^22 - 4: R [., K] | X [., D] | Y [., E] side by side -------------------------------------------
    # (K = 64, D = 16, Y == X: 136 pairs in five tiles, weighted_outer_kernel<2, 5>; K = 8, D = E = 16: <1, 8>)
    case("wouter-sym", "wouter", 300, 80, LD22, 1 << 22, 64, sym=True, K=64, D=16, E=16),
    case("wouter-xy", "wouter", 300, 40, LD22, 1 << 22, 64, sym=False, K=8, D=16, E=16),
    # ---- the 32-row kernels: 40 rows at 2^25 - 4 ------------------------------------------------------------------
    case("mog-D16", "mog", 40, 16, LD25, 1 << 25, 32, L16, D=16),
    case("mog-D5", "mog", 40, 5, LD25, 1 << 25, 32, L16, D=5),
    case("mog-bx-D16", "mog", 40, 16, LD25, 1 << 25, 32, L16, dict(mfma_split=2), D=16),
    case("gsr-K16", "gsr", 40, 16, LD25, 1 << 25, 32, L16, K=16, N=12),
    case("gsr-K40", "gsr", 40, 40, LD25, 1 << 25, 32, L16, K=40, N=8),
    case("gsr-K64", "gsr", 40, 64, LD25, 1 << 25, 32, L16, K=64, N=64),
    case("gss-K24", "gss", 40, 24, LD25, 1 << 25, 32, L16, K=24, N=12, bias=False),
    case("gss-K24-bias", "gss", 40, 24, LD25, 1 << 25, 32, L16, K=24, N=12, bias=True),
    # ---- S cases: total span past 2^32 at a moderate stride ---------------------------------------------------------
    case("gram-D64", "gram", 4100, 64, 327680, 1 << 25, 32, options=dict(mfma_split=2), D=64),
    case("gram-D256", "gram", 4100, 256, 327680, 1 << 25, 32, options=dict(mfma_split=2), D=256),
    # (24 short rows, K = 256: gemm_skinny_nt_kernel<2, 16>; 8 short rows, K = 64: <1, 4>)
    case("skinny-nt", "skinny_nt", 4100, 256, 327680, 1 << 26, 32, swapped=False, small=24, K=256),
    case("skinny-nt-swapped", "skinny_nt", 4100, 64, 327680, 1 << 26, 32, swapped=True, small=8, K=64),
    case("skinny-tn", "skinny_tn", 16384, 64, 81920, 1 << 26, 32, ragged=False),
    # ---- the weighted, grouped and learned-scalar passes (tests/_span_borrowed.py): 24 rows at 2^26 - 4 ---------------
    case("glm-obs-mfma-D256", "glm_obs", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8, link="poisson"),
    case("glm-obs-valu-D64", "glm_obs", 24, 64, LD26, 1 << 26, 8, ragged=False, D=64, S=8, link="logistic"),
    case("glm-groups-D256", "glm_groups", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8, link="logistic", J=5),
    case("glm-nb-D256", "glm_nb", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8),
    case("weibull-interval-D256", "weibull_interval", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8),
    case("ordinal-ldx", "ordinal", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8, K=5, spread="X"),
    # the draws Z [S, D + K - 1] spread instead: 24 draws are three launches of eight (D = 252: the 256 columns of Z that
    # the buffer has room for behind its last row)
    case("ordinal-ldz", "ordinal", 24, 256, LD26, 1 << 26, 8, ragged=False, B=24, D=252, S=24, K=5, spread="Z"),
    case("predict-offset-D256", "predict_offset", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8, family="logistic"),
    case("predict-groups-D256", "predict_groups", 24, 256, LD26, 1 << 26, 16, L16, D=256, S=8, family="poisson", J=5),
    # ---- bsc_lda_sstats (70 documents, V = 1028, K = 128): each inequality of the stream kernel, just below --------
    _lda_case("C", "below"), _lda_case("Th", "below"), _lda_case("Bt", "below"),
    # ... and on split operands (option mfma_split; bsc_lda_sstats_bound where `bound`): lda_sstats_bx2_kernel,
    # lda_sstats_bx2_bound_kernel, lda_sstats_bx3_bound_kernel
    _lda_case("Bt", "below", "-bx2", dict(mfma_split=2)), _lda_case("C", "below", "-bx2-bound", dict(mfma_split=2), True),
    _lda_case("Th", "below", "-bx3-bound", dict(mfma_split=3), True),
]
# a DECLINING gate just above: the general kernel must answer, and be right
DECLINED = [_lda_case("C", "above"), _lda_case("Th", "above"), _lda_case("Bt", "above")]
LDX = r"ldx=\d+ must be >= D, % 4 == 0 and < 2\^26"
ABOVE = [
    # 20 rows: 19 * 2^26 + 256 floats still fit the buffer
    case("blr", "blr", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, message=r"bsc_blr_data_pass: ldx=\d+ must be >= D, % 4 == 0"),
    case("glm", "glm", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, link="logistic", message=r"ldx=\d+ must be >= D, % 4 == 0"),
    case("softmax", "softmax", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=4, K=5, message=r"ldx=\d+ must be >= D, % 4 == 0"),
    case("predict", "predict", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, family="logistic",
         message=r"ldx=\d+ must be >= D, % 4 == 0"),
    case("softmax-predict", "softmax_predict", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=7, K=3,
         message=r"ldx=\d+ must be >= D, % 4 == 0"),
    case("bbvi", "bbvi", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=64, message=r"bad ldx=\d+"),
    case("wouter", "wouter", 300, 40, 1 << 22, 1 << 22, 64, sym=False, K=8, D=16, E=16,
         message=r"bsc_weighted_outer: leading dimensions must be below 2\^22"),
    case("mog", "mog", 40, 16, 1 << 25, 1 << 25, 32, D=16, message=r"bsc_mog_estep: bad ldx=\d+"),
    case("gsr", "gsr", 40, 16, 1 << 25, 1 << 25, 32, K=16, N=12, message=r"bsc_gemm_softmax_rows: lda=\d+"),
    case("gss", "gss", 40, 24, 1 << 25, 1 << 25, 32, K=24, N=12, bias=False, message=r"bsc_gemm_softmax_stats: lda=\d+"),
    case("glm-obs", "glm_obs", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, link="poisson", message=r"bsc_glm_data_pass_obs: " + LDX),
    case("glm-groups", "glm_groups", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, link="logistic", J=5,
         message=r"bsc_glm_data_pass_groups: " + LDX),
    case("glm-nb", "glm_nb", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, message=r"bsc_glm_nb_data_pass: " + LDX),
    case("weibull-interval", "weibull_interval", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8,
         message=r"bsc_glm_weibull_data_pass_interval: " + LDX),
    case("ordinal-ldx", "ordinal", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, K=5, spread="X",
         message=r"bsc_glm_ordinal_data_pass: " + LDX),
    case("ordinal-ldz", "ordinal", 20, 256, 1 << 26, 1 << 26, 8, B=24, D=252, S=20, K=5, spread="Z",
         message=r"bsc_glm_ordinal_data_pass: ldz=\d+ must be >= D \+ K - 1 and < 2\^26"),
    case("predict-offset", "predict_offset", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, family="logistic",
         message=r"bsc_predict_pass_offset: " + LDX),
    case("predict-groups", "predict_groups", 20, 256, 1 << 26, 1 << 26, 16, D=256, S=8, family="poisson", J=5,
         message=r"bsc_predict_pass_groups: " + LDX),
]
EXECUTOR = [("below", LD25), ("above", 1 << 25)]


def span_floats(c):
    return (c["rows"] - 1) * c["ld"] + c["width"]


def test_span_cases_reach_what_they_claim():
    """(Needs no device.)  From each case's numbers alone: the documented inequality holds below and fails above,
    ld % 4 == 0, the span fits the shared buffer and 8 GiB, and the case reaches the offsets it claims."""
    assert WIDE_FLOATS * 4 < CAP_BYTES
    ids = [c["id"] for c in BELOW]
    assert len(set(ids)) == len(ids)
    for c in BELOW + ABOVE + DECLINED + [case(n, "gsr", 40, 24, ld, 1 << 25, 32) for n, ld in EXECUTOR]:
        below = c in BELOW or c["id"] == "below"
        assert (c["ld"] < c["limit"]) == below, c["id"]
        if c["entry"] == "lda":                        # the three inequalities as the dispatcher writes them
            assert borrowed.lda_holds(c["spread"], c["ld"]) == below, c["id"]
            assert borrowed.lda_holds(c["spread"], c["limit"] - 1) and not borrowed.lda_holds(c["spread"], c["limit"])
        assert c["ld"] % 4 == 0 and c["ld"] >= c["width"], c["id"]
        assert span_floats(c) <= WIDE_FLOATS and span_floats(c) * 4 < CAP_BYTES, c["id"]
        assert c["rows"] > c["tile"] and (c["rows"] % c["tile"] != 0) == c["ragged"], c["id"]   # more than one tile
        if not below:
            assert c["ld"] - 4 < c["limit"] <= c["ld"], c["id"]                    # the first multiple of 4 past the gate
            continue
        if "total32" in c["claims"]:
            assert span_floats(c) * 4 >= 1 << 32, c["id"]
        if "tile31" in c["claims"]:
            assert (c["tile"] - 1) * c["ld"] * 4 >= 1 << 31, c["id"]
        if c["limit"] == 1 << 25:                      # the 32-row kernels: the last row's lane offset fits 32 bits
            assert (31 * c["ld"] + c["width"]) * 4 < 1 << 32, c["id"]
    # the cases just below a documented limit sit at limit - 4
    for c in BELOW:
        if c["rows"] in (24, 40, 300):
            assert c["ld"] == c["limit"] - 4, c["id"]
        assert c["limit"] - 4 <= c["ld"] or c["rows"] >= 1100, c["id"]             # (the S cases are far below theirs)
    # what the old limit of the 32-row kernels admitted: at 2^26 - 4 the offset of row 17 wraps to byte 2^28 - 272
    assert (17 * LD26 * 4) % (1 << 32) == (1 << 28) - 272 and 16 * LD26 * 4 < 1 << 32
    # the clamped / unclamped crossing of the B = 1100 case: descriptors are clamped while the rows left span > 4 GiB
    c = next(c for c in BELOW if c["id"] == "blr-q-B1100-ld2^20")
    clamped = [r0 for r0 in range(0, c["rows"], 16) if ((c["rows"] - r0 - 1) * c["ld"] + 256) * 4 > 0xFFFFFFFF]
    assert 2 <= len(clamped) < (c["rows"] + 15) // 16 - 2


# =====================================================================================================
# the wide buffer and the placement of a case in it
# =====================================================================================================
@pytest.fixture(scope="module")
def wide(ctx):
    import torch
    buf = torch.full((WIDE_FLOATS,), float("nan"), dtype=torch.float32, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def alt(ctx):
    """alt(name=value) -> a second Context on the session context's device and stream (tests/test_view_routes_gpu.py's)."""
    from bayesic_amd.device import Context
    made = {}

    def get(**options):
        if not options:
            return ctx
        key = tuple(sorted(options.items()))
        if key not in made:
            made[key] = Context(ctx.device_index, stream=ctx.stream, options=options)
        return made[key]

    yield get
    for c in made.values():
        c.close()


@contextlib.contextmanager
def spread(wide, A, ld):
    """The rows of A [rows, width] ld floats apart from the start of `wide`; NaN again afterwards."""
    import torch
    rows, width = A.shape
    assert (rows - 1) * ld + width <= wide.numel()
    view = torch.as_strided(wide, (rows, width), (ld, 1))
    src = torch.from_numpy(np.ascontiguousarray(A)).to(wide.device)
    if rows <= 64:
        for r in range(rows):
            wide[r * ld:r * ld + width].copy_(src[r])
    else:
        view.copy_(src)
    try:
        yield view
    finally:
        if rows <= 64:
            for r in range(rows):
                wide[r * ld:r * ld + width].fill_(float("nan"))
        else:
            view.fill_(float("nan"))


_OUTPUTS = []                                   # the output tensors of the run in flight (test_refused reads them back)


def _nan(ctx, shape, dtype=None):
    import torch
    t = torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype or torch.float32,
                   device=ctx.device)
    _OUTPUTS.append(t)
    return t


def _rs(c):
    return np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])) % (2 ** 31))


def _worst(name, err, bound):
    w = float(np.max(np.asarray(err) / (np.asarray(bound) + 1e-300)))
    assert w <= 1.0, (name, w)
    return "%s %.3g" % (name, w)


# =====================================================================================================
# per entry point: make(c) -> host data with "M" the [rows, width] matrix that is spread;
# run(cx, ptr, ld, c, d) -> name -> numpy (outputs NaN-prefilled); check(c, d, got) -> the printed figures
# =====================================================================================================
def blr_make(c):
    rs = _rs(c)
    X = rs.standard_normal((c["rows"], c["D"])).astype(F32)
    return dict(M=X, y=rs.standard_normal(c["rows"]).astype(F32), W=(rs.standard_normal((c["S"], c["D"])) / 8).astype(F32))


def blr_run(cx, ptr, ld, c, d):
    import torch
    S, D = c["S"], c["D"]
    Q, G = _nan(cx, S, torch.float64), _nan(cx, (S, D), torch.float64)
    cx.call("bsc_blr_data_pass", ptr, ld, cx.to_device(d["y"]), c["rows"], D, cx.to_device(d["W"]), S, Q, G)
    cx.sync()
    return dict(Q=Q.cpu().numpy(), G=G.cpu().numpy())


def blr_check(c, d, got):
    from oracle import svi
    X, y, W = d["M"], d["y"], d["W"]
    q_ref, g_ref = svi.blr_data_pass(X, y, W)
    X64 = X.astype(F64)
    size = np.abs(y.astype(F64))[:, None] + np.abs(X64) @ np.abs(W.astype(F64)).T
    scale = np.sqrt(q_ref)[:, None] * np.sqrt((X64 ** 2).sum(0))[None, :] + 1e-12
    g_size = (size[:, :, None] * np.abs(X64)[:, None, :]).sum(0)
    return [_worst("Q", np.abs(got["Q"] - q_ref), 3e-6 * (q_ref + 1e-1 * (size ** 2).sum(0))),
            _worst("G", np.abs(got["G"] - g_ref), 2e-5 * scale + 3e-7 * g_size)]


def glm_make(c):
    import test_glm_gpu as glm_t
    X, y, W = glm_t._inputs(c["link"], c["rows"], c["D"], c["S"], seed=len(c["id"]) + c["D"])
    return dict(M=X, y=y, W=W)


def glm_run(cx, ptr, ld, c, d):
    import torch
    import test_glm_gpu as glm_t
    S, D = c["S"], c["D"]
    ell, G = _nan(cx, S, torch.float64), _nan(cx, (S, D), torch.float64)
    cx.call("bsc_glm_data_pass", glm_t.CODE[c["link"]], ptr, ld, cx.to_device(d["y"]), c["rows"], D, cx.to_device(d["W"]), S,
            ell, G)
    cx.sync()
    return dict(ell=ell.cpu().numpy(), G=G.cpu().numpy())


def glm_check(c, d, got):
    import _glm_ref as glm
    X, y, W = d["M"], d["y"], d["W"]
    ell_r, G_r = glm.glm_data_pass(c["link"], X, y, W)
    L = X.astype(F64) @ W.astype(F64).T
    if c["link"] == "poisson":
        assert np.abs(L).max() <= 4.0
    A, _ = glm.log_partition(c["link"], L)
    bound = (np.abs(y.astype(F64)[:, None] * L) + A + 1.0).sum(axis=0)
    return [_worst("ell", np.abs(got["ell"] - ell_r), 2e-5 * bound + 1e-12),
            _worst("G", np.abs(got["G"] - G_r), 1e-4 * np.abs(G_r) + 1e-4 * np.abs(G_r).max())]


def softmax_make(c):
    import test_softmax_regression_gpu as softmax_t
    X, y, W = softmax_t._inputs(c["rows"], c["D"], c["K"], c["S"], c["K"] + c["S"])
    return dict(M=X, y=y, W=W)


def softmax_run(cx, ptr, ld, c, d):
    import torch
    S, D, K = c["S"], c["D"], c["K"]
    ell, G = _nan(cx, S, torch.float64), _nan(cx, (S, K, D), torch.float64)
    cx.call("bsc_softmax_data_pass", ptr, ld, cx.to_device(np.asarray(d["y"], np.int32)), c["rows"], D, K, cx.to_device(d["W"]),
            S, ell, G)
    cx.sync()
    return dict(ell=ell.cpu().numpy(), G=G.cpu().numpy())


def softmax_check(c, d, got):
    import _softmax_ref as sref
    X, y, W = d["M"], d["y"], d["W"]
    ell_r, G_r = sref.softmax_data_pass(X, y, W)
    gmax = np.abs(G_r).max()
    return [_worst("ell", np.abs(got["ell"] - ell_r), 2e-5 * sref.ell_bound(X, y, W) + 1e-12),
            _worst("G", np.abs(got["G"] - G_r), 1e-4 * np.abs(G_r) + 1e-4 * gmax)]


def predict_make(c):
    import test_predict_gpu as predict_t
    X, y, W, logvar = predict_t._inputs(c["family"], c["rows"], c["D"], c["S"], 3)
    return dict(M=X, y=y, W=W, logvar=logvar)


def predict_run(cx, ptr, ld, c, d):
    import torch
    import _predict_ref as pref
    B, D, S = c["rows"], c["D"], c["S"]
    out = {k: _nan(cx, B) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = _nan(cx, 1, torch.float64)
    lvd = None if d["logvar"] is None else cx.to_device(d["logvar"])
    cx.call("bsc_predict_pass", pref.CODE[c["family"]], ptr, ld, cx.to_device(d["y"]), B, D, cx.to_device(d["W"]), lvd, S,
            out["mean"], out["var"], out["lpd"], out["lpd_sum"])
    cx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def predict_check(c, d, got):
    import _predict_ref as pref
    want = pref.predict(c["family"], d["M"], d["W"], d["logvar"], d["y"])
    bnd = pref.bounds(c["family"], d["M"], d["W"], d["logvar"], d["y"])
    return [_worst(k, np.abs(got[k] - want[k]), bnd[k]) for k in ("mean", "var", "lpd", "lpd_sum")]


def softmax_predict_make(c):
    d = softmax_make(c)
    d["y"] = d["y"].copy()
    d["y"][::9] = -1                                         # rows with a label outside the classes score 0
    return d


def softmax_predict_run(cx, ptr, ld, c, d):
    import torch
    B, D, S, K = c["rows"], c["D"], c["S"], c["K"]
    prob, lpd, lpd_sum = _nan(cx, B * K), _nan(cx, B), _nan(cx, 1, torch.float64)
    cx.call("bsc_softmax_predict_pass", ptr, ld, cx.to_device(np.asarray(d["y"], np.int32)), B, D, K, cx.to_device(d["W"]), S,
            prob, lpd, lpd_sum)
    cx.sync()
    return dict(prob=prob.cpu().numpy().reshape(B, K), lpd=lpd.cpu().numpy(), lpd_sum=lpd_sum.cpu().numpy())


def softmax_predict_check(c, d, got):
    import _softmax_ref as sref
    r, b = sref.predict(d["M"], d["W"], d["y"]), sref.predict_bounds(d["M"], d["W"], d["y"])
    assert (got["lpd"][::9] == 0.0).all()
    assert abs(got["lpd_sum"][0] - r["lpd_sum"]) <= b["lpd_sum"]
    return [_worst("prob", np.abs(got["prob"] - r["prob"]), b["prob"]),
            _worst("lpd", np.abs(got["lpd"] - r["lpd"]), b["lpd"])]


def bbvi_make(c):
    rs = _rs(c)
    N, D, S, G = c["rows"], c["D"], c["S"], 7
    return dict(M=rs.standard_normal((N, D)).astype(F32), y=(rs.uniform(size=N) < 0.4).astype(F32),
                g=rs.randint(G, size=N).astype(np.int32), Wz=(rs.standard_normal((S, D)) / math.sqrt(D)).astype(F32),
                Bz=rs.standard_normal((G, S)).astype(F32))


def bbvi_run(cx, ptr, ld, c, d):
    import torch
    S = c["S"]
    ell = _nan(cx, S, torch.float64)
    cx.call("bsc_logreg_bbvi_loglik", ptr, ld, cx.to_device(d["y"]), cx.to_device(d["g"]), c["rows"], c["D"], d["Bz"].shape[0],
            cx.to_device(d["Wz"]), cx.to_device(d["Bz"]), S, ell)
    cx.sync()
    return dict(ell=ell.cpu().numpy())


def bbvi_check(c, d, got):
    from oracle import svi
    want = svi.logreg_loglik(d["M"], d["y"], d["g"], d["Wz"], d["Bz"])
    L = np.abs(d["M"].astype(F64) @ d["Wz"].astype(F64).T + d["Bz"].astype(F64)[d["g"]])
    return [_worst("ell", np.abs(got["ell"] - want), 2e-5 * (L + 1.0).sum(axis=0) + 1e-9)]


def wouter_make(c):
    return dict(M=_rs(c).standard_normal((c["rows"], c["K"] + c["D"] + (0 if c["sym"] else c["E"]))).astype(F32))


def wouter_run(cx, ptr, ld, c, d):
    K, D, E = c["K"], c["D"], c["E"]
    out = _nan(cx, (K, D, E))
    x = ptr + 4 * K
    y = x if c["sym"] else x + 4 * D
    cx.call("bsc_weighted_outer", ptr, ld, x, ld, y, ld, c["rows"], K, D, E, 1.0, out)
    cx.sync()
    return dict(out=out.cpu().numpy())


def wouter_check(c, d, got):
    M = d["M"].astype(F64)
    R, X = M[:, :c["K"]], M[:, c["K"]:c["K"] + c["D"]]
    Y = X if c["sym"] else M[:, c["K"] + c["D"]:]
    want = np.einsum("nk,nd,ne->kde", R, X, Y)
    bound = np.einsum("nk,nd,ne->kde", np.abs(R), np.abs(X), np.abs(Y))
    if c["sym"]:
        npt.assert_array_equal(got["out"], got["out"].transpose(0, 2, 1))
    return [_worst("out", np.abs(got["out"] - want), 2e-5 * bound + 1e-30)]


def mog_make(c):
    import test_view_routes_gpu as vr
    X, Wmat, cvec = vr.mog_data(dict(id=c["id"], N=c["rows"], D=c["D"], K=5))
    return dict(M=X, Wmat=Wmat, cvec=cvec)


def mog_run(cx, ptr, ld, c, d):
    import torch
    D, K = c["D"], 5
    stats, lse = _nan(cx, (K, 1 + 2 * D), torch.float64), _nan(cx, 1, torch.float64)
    cx.call("bsc_mog_estep", ptr, ld, c["rows"], D, K, cx.to_device(d["Wmat"]), cx.to_device(d["cvec"]), stats, lse)
    cx.sync()
    return dict(stats=stats.cpu().numpy(), lse=lse.cpu().numpy())


def mog_check(c, d, got):
    from oracle import svi
    X = d["M"]
    s, l = svi.mog_local_step(X, d["Wmat"], d["cvec"])
    X64 = np.abs(X.astype(F64))
    scale = np.concatenate([[max(c["rows"], 1)], X64.sum(0) + 1e-9, (X64 ** 2).sum(0) + 1e-9])
    split = bool(c["options"].get("mfma_split"))
    tol, rtol = (2e-5, 2e-6) if split else (3e-5, 3e-6)
    return [_worst("stats", np.abs(got["stats"] - s), tol * scale[None, :] + 1e-9),
            _worst("lse", abs(got["lse"][0] - l), rtol * abs(l) + 1e-4)]


def gs_make(c):
    rs = _rs(c)
    d = dict(M=rs.standard_normal((c["rows"], c["K"])).astype(F32), B=(rs.standard_normal((c["K"], c["N"])) * 1.5).astype(F32))
    if c.get("bias"):
        d["bias"] = rs.standard_normal(c["N"]).astype(F32)
    return d


def gsr_run(cx, ptr, ld, c, d):
    rows, K, N = c["rows"], c["K"], c["N"]
    R, lse, cross = _nan(cx, (rows, N)), _nan(cx, rows), _nan(cx, rows)
    cx.call("bsc_gemm_softmax_rows", ptr, ld, rows, K, cx.to_device(d["B"]), N, 1, N, 1.0, R, N, lse, cross)
    cx.sync()
    return dict(R=R.cpu().numpy(), lse=lse.cpu().numpy(), cross=cross.cpu().numpy())


def gss_run(cx, ptr, ld, c, d):
    import torch
    rows, K, N = c["rows"], c["K"], c["N"]
    ldst = K + 1
    R, st, tot = _nan(cx, (rows, N)), _nan(cx, (N, ldst)), _nan(cx, 1, torch.float64)
    bias = cx.to_device(d["bias"]) if c["bias"] else None
    cx.call("bsc_gemm_softmax_stats", ptr, ld, rows, K, cx.to_device(d["B"]), N, 1, N, 1.0, bias, R, N, st, ldst, tot)
    cx.sync()
    return dict(R=R.cpu().numpy(), stats=st.cpu().numpy(), lse_sum=tot.cpu().numpy())


def _gs_reference(d):
    A = d["M"].astype(F64)
    logits = A @ d["B"].astype(F64) + (d["bias"].astype(F64)[None, :] if "bias" in d else 0.0)
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    return A, logits, e / e.sum(1, keepdims=True), (m + np.log(e.sum(1, keepdims=True)))[:, 0]


def gsr_check(c, d, got):
    A, logits, want, lse = _gs_reference(d)
    cross = (want * logits).sum(1)
    scale = np.abs(logits).max() + 1.0
    return [_worst("R", np.abs(got["R"] - want), 2e-5 * np.abs(want) + 2e-6),
            _worst("lse", np.abs(got["lse"] - lse), 1e-5 * scale), _worst("cross", np.abs(got["cross"] - cross), 2e-5 * scale)]


def gss_check(c, d, got):
    A, logits, want, lse = _gs_reference(d)
    K = c["K"]
    s_ref, s_bound = want.T @ A, want.T @ np.abs(A)
    figs = [_worst("R", np.abs(got["R"] - want), 2e-5 * np.abs(want) + 2e-6),
            _worst("stats", np.abs(got["stats"][:, :K] - s_ref), 3e-6 * s_bound + 1e-6),
            _worst("lse_sum", abs(got["lse_sum"][0] - lse.sum()), 2e-6 * abs(lse.sum()))]
    if c["bias"]:                                            # the column sums of R, the statistic of the ones column
        figs.append(_worst("colsum", np.abs(got["stats"][:, K] - want.sum(0)), 3e-6 * want.sum(0) + 1e-6))
    else:
        assert np.isnan(got["stats"][:, K]).all()            # ldst = K + 1: the spare column is not written
    return figs


def gram_make(c):
    return dict(M=(_rs(c).standard_normal((c["rows"], c["D"])) + 0.3).astype(F32))


def gram_run(cx, ptr, ld, c, d):
    D, N = c["D"], c["rows"]
    out = _nan(cx, (D, D))
    cx.call("bsc_gemm_strided_batched", 0, 1, D, D, N, ptr, 0, 1, ld, ptr, 0, ld, 1, out, 0, D, 1)
    cx.sync()
    return dict(C=out.cpu().numpy())


def gram_check(c, d, got):
    X = d["M"].astype(F64)
    n2 = np.sqrt((X ** 2).sum(0))
    npt.assert_array_equal(got["C"], got["C"].T)
    return [_worst("C", np.abs(got["C"] - X.T @ X), 2e-5 * n2[:, None] * n2[None, :])]


def skinny_nt_make(c):
    rs = _rs(c)
    return dict(M=rs.standard_normal((c["rows"], c["K"])).astype(F32),
                small=rs.standard_normal((c["small"], c["K"])).astype(F32))


def skinny_nt_run(cx, ptr, ld, c, d):
    n, K, m = c["rows"], c["K"], c["small"]
    sm = cx.to_device(d["small"])                                # [m, K]
    if c["swapped"]:                                             # A = M [n, K] long, B = small^T [K, m]
        out = _nan(cx, (n, m))
        cx.call("bsc_gemm_strided_batched", 0, 1, n, m, K, ptr, 0, ld, 1, sm, 0, 1, K, out, 0, m, 1)
    else:                                                        # A = small [m, K], B = M^T [K, n]
        out = _nan(cx, (m, n))
        cx.call("bsc_gemm_strided_batched", 0, 1, m, n, K, sm, 0, K, 1, ptr, 0, 1, ld, out, 0, n, 1)
    cx.sync()
    return dict(C=out.cpu().numpy())


def skinny_nt_check(c, d, got):
    M, s = d["M"].astype(F64), d["small"].astype(F64)
    want, bound = (M @ s.T, np.abs(M) @ np.abs(s).T) if c["swapped"] else (s @ M.T, np.abs(s) @ np.abs(M).T)
    return [_worst("C", np.abs(got["C"] - want), 1e-5 * bound + 1e-30)]


def skinny_tn_make(c):
    rs = _rs(c)
    return dict(M=rs.standard_normal((c["rows"], 64)).astype(F32), small=rs.standard_normal((8, c["rows"])).astype(F32))


def skinny_tn_run(cx, ptr, ld, c, d):
    K = c["rows"]                                                # A = small [8, K] k-contiguous, B = M [K, 64] with sb_k = ld
    out = _nan(cx, (8, 64))
    cx.call("bsc_gemm_strided_batched", 0, 1, 8, 64, K, cx.to_device(d["small"]), 0, K, 1, ptr, 0, ld, 1, out, 0, 64, 1)
    cx.sync()
    return dict(C=out.cpu().numpy())


def skinny_tn_check(c, d, got):
    M, s = d["M"].astype(F64), d["small"].astype(F64)
    return [_worst("C", np.abs(got["C"] - s @ M), 1e-5 * (np.abs(s) @ np.abs(M)) + 1e-30)]


ENTRY = {
    "blr": (blr_make, blr_run, blr_check), "glm": (glm_make, glm_run, glm_check),
    "softmax": (softmax_make, softmax_run, softmax_check), "predict": (predict_make, predict_run, predict_check),
    "softmax_predict": (softmax_predict_make, softmax_predict_run, softmax_predict_check),
    "bbvi": (bbvi_make, bbvi_run, bbvi_check), "wouter": (wouter_make, wouter_run, wouter_check),
    "mog": (mog_make, mog_run, mog_check), "gsr": (gs_make, gsr_run, gsr_check), "gss": (gs_make, gss_run, gss_check),
    "gram": (gram_make, gram_run, gram_check), "skinny_nt": (skinny_nt_make, skinny_nt_run, skinny_nt_check),
    "skinny_tn": (skinny_tn_make, skinny_tn_run, skinny_tn_check),
}


def _with_outputs(run):
    return lambda cx, ptr, ld, c, d: run(cx, ptr, ld, c, d, _OUTPUTS)


ENTRY.update({name: (make, _with_outputs(run), check) for name, (make, run, check) in borrowed.ENTRY.items()})


def run_spread(cx, wide, c, d):
    _, run, _ = ENTRY[c["entry"]]
    del _OUTPUTS[:]
    with spread(wide, d["M"], c["ld"]) as view:
        return run(cx, view.data_ptr(), c["ld"], c, d)


def run_compact(cx, c, d):
    _, run, _ = ENTRY[c["entry"]]
    del _OUTPUTS[:]
    compact = cx.to_device(np.ascontiguousarray(d["M"]))
    assert compact.data_ptr() % 16 == 0
    return run(cx, compact.data_ptr(), d["M"].shape[1], c, d)


# =====================================================================================================
# the tests
# =====================================================================================================
pytest_gpu = pytest.mark.gpu


@pytest_gpu
@pytest.mark.parametrize("c", BELOW, ids=[c["id"] for c in BELOW])
def test_below_gate(ctx, alt, wide, c):
    make, _, check = ENTRY[c["entry"]]
    cx = alt(**c["options"])
    d = make(c)
    assert d["M"].shape == (c["rows"], c["width"])
    got = run_spread(cx, wide, c, d)
    figures = check(c, d, got)
    print("%s rows=%d ld=%d: worst error / bound  %s" % (c["id"], c["rows"], c["ld"], "  ".join(figures)))
    dense = run_compact(cx, c, d)
    for k in got:
        npt.assert_array_equal(got[k], dense[k], err_msg="%s: %s differs from the compact run" % (c["id"], k))


@pytest_gpu
@pytest.mark.parametrize("c", ABOVE, ids=[c["id"] for c in ABOVE])
def test_refused(ctx, wide, c):
    from bayesic_amd._ffi import BayesicHipError
    make, run, _ = ENTRY[c["entry"]]
    d = make(c)
    del _OUTPUTS[:]
    with spread(wide, d["M"], c["ld"]) as view:
        with pytest.raises(BayesicHipError, match=c["message"]):
            run(ctx, view.data_ptr(), c["ld"], c, d)
        ctx.sync()
    assert _OUTPUTS, "the runner allocated no output"
    for t in _OUTPUTS:                           # NaN-prefilled by the runner before the call that raised
        assert bool(t.isnan().all()), "an output was written by a refused call"
    # the context stays usable: the same rows just below the gate
    ok = dict(c, ld=c["limit"] - 4)
    ENTRY[c["entry"]][2](ok, d, run_spread(ctx, wide, ok, d))


@pytest_gpu
@pytest.mark.parametrize("c", DECLINED, ids=[c["id"] for c in DECLINED])
def test_declined_takes_the_general_route(ctx, wide, c):
    make, _, check = ENTRY[c["entry"]]
    d = make(c)
    figures = check(c, d, run_spread(ctx, wide, c, d))
    print("%s rows=%d ld=%d: worst error / bound  %s" % (c["id"], c["rows"], c["ld"], "  ".join(figures)))


@pytest_gpu
@pytest.mark.parametrize("side,ld", EXECUTOR, ids=[s for s, _ in EXECUTOR])
def test_softmax_of_a_product_on_a_far_view(ctx, wide, side, ld):
    """A Categorical node's update softmax_rows(X . Y) with the rows of X 2^25 - 4 / 2^25 floats apart: ONE
    bsc_gemm_softmax_rows launch below the limit; at it the executor does not call the fused entry point (which would
    refuse) but takes the product and bsc_softmax_rows.  test_view_routes_gpu's test of the same route, its tolerances."""
    from bayesic_amd.algebra import dot, var
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from test_fusion_gpu import Counting
    rs = np.random.RandomState(10)
    rows, K, N = 40, 24, 12
    X_ = rs.standard_normal((rows, K)).astype(F32)
    Y_ = (rs.standard_normal((K, N)) * 1.5).astype(F32)
    _, logits, want, lse_ref = _gs_reference(dict(M=X_, B=Y_))
    be = DeviceBackend(ctx)
    with spread(wide, X_, ld) as view:
        with Counting(ctx) as c:
            R, lse, cross, _ = be.evaluate_softmax_rows(dot(var("X", ndim=2), var("Y", ndim=2)),
                                                        dict(X=view, Y=ctx.to_device(Y_)))
        ctx.sync()
        R, lse = R.cpu().numpy(), lse.cpu().numpy()
    if side == "below":
        assert c.count("bsc_gemm_softmax_rows") == 1 and c.count("bsc_softmax_rows") == 0, c.calls
    else:
        assert c.count("bsc_gemm_softmax_rows") == 0 and c.count("bsc_softmax_rows") == 1 and \
            c.count("bsc_gemm_strided_batched") + c.count("bsc_gemm_epilogue") == 1, c.calls
    npt.assert_allclose(R, want, rtol=2e-5, atol=2e-6)
    npt.assert_allclose(lse, lse_ref, rtol=0, atol=1e-5 * (np.abs(logits).max() + 1.0))
