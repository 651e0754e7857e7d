"""Entry points that pick a kernel from the ADDRESS ARITHMETIC of their operands, crossed on both sides of
each gate: operands are views of wider buffers (tests/_views.py) -- base offsets of 1..3 elements, leading
dimensions with every remainder mod 4, transposed and inner-stride-2 views, batch strides that are not a
multiple of four -- against float64 numpy on the same float32 values.  Input buffers are NaN outside the
view (a read outside poisons the result); output buffers carry a sentinel whose bits are compared after
every call (a 16-byte store over a ragged edge is seen even where it lands in a row gap).

Tolerances are the suite's own, per entry point, not widened: GEMM / GEMV / skinny <= 1e-5 (|A| @ |B|)
(test_shape_sweep_gpu.test_gemm_strided_sweep); the epilogue rtol 3e-5 on positive operands
(test_fusion_gpu.test_gemm_consumers_fold_into_the_store); the producer-fused product rtol 2e-4, atol 2e-5 of
the largest entry (test_fusion_gpu.test_producers_fold_into_the_operand_reads); softmax rows rtol 3e-5 and lse
1e-6 (test_softmax_gpu); the Dirichlet expectation rtol 2e-6 and its bound rtol 1e-11, atol 1e-9 (test_lda_gpu);
the LDA statistic rtol 3e-5, atol 1e-6 and its words term 3e-6 of sum C |log phinorm| (test_lda_gpu); the mixture
E-step 3e-5 * scale (test_shape_sweep_gpu.test_mog_estep_sweep); bsc_suffstats_normal rtol 1e-13 (test_blr_gpu);
sums of positive terms rtol 1e-5 = 84 eps_f32 * sum|terms| (test_fusion_gpu: sum(exp(X) * Y), rtol 1e-5);
element-wise maps and the float32 natural-gradient step (three roundings of positive terms) rtol 1e-6, atol
1e-6 (test_fusion_gpu: X * u + 1).

One row per gate: the route function or predicate that holds it (names as in the source file, no line numbers),
a case that takes the 16-byte / LDS-DMA side and one that takes the fall-back (ids as pytest prints them; kernel
names as a kernel trace prints them, profiles/view_routes_kernel_stats.csv).
WHAT THE TRACE SHOWS: where the two sides are DIFFERENT kernels (marked [K]) both names have a non-zero count in the
CSV.  Where the gate is a branch inside ONE kernel (marked [B]) the trace cannot tell the sides apart: that both
ran follows from the dispatcher / kernel source at the place named and from the cases' layouts, nothing more.

  [K] bsc_gemm.hip gemm_stream: dma_ok, alignment       gemm_f32_stream_kernel <- test_gemm[plain-256x384x160-b1-ctl]
                                                        gemm_f32_mfma_kernel <- test_gemm[plain-256x384x160-b1-Aoff1]
  [K] bsc_gemm.hip gemm_stream: dma_ok, lane offsets    gemm_f32_stream_kernel <- test_span_gates[gemm-kcontig-below], [gemm-mcontig-below]
                                                        gemm_f32_mfma_kernel <- test_span_gates[gemm-kcontig-above], [gemm-mcontig-above]
  [K] bsc_gemm.hip gemm_tile: dma_ok (the same          gemm_f32_dma_kernel: not reached by the cases of this file -- with the default
      predicate), after short_k_plain or gemm_dma = 1   gemm_dma = 2 every layout that passes dma_ok has left by gemm_stream, and these shapes
                                                        do not meet short_k_plain.  Reached by test_algebra_gpu.py:
                                                        test_gemm_operands_by_lds_dma_all_layouts (its context with gemm_dma = 1: gemm_f32_dma_kernel
                                                        where dma_ok holds, gemm_f32_mfma_kernel where it does not: 130x257x1000, 257x129x20) and
                                                        test_gemm_short_contraction_over_many_full_tiles[at-the-gate] (short_k_plain at default
                                                        settings; [below-the-gate]: gemm_f32_stream_kernel) -- profiles/gemm_tile_route_kernel_stats.csv
  [B] bsc_gemm.hip gemm_tile: vec_ok / g.fast           gemm_f32_mfma_kernel <- test_gemm[plain-129x257x33-b1-ctl] (16-byte loads)
                                                        the same kernel <- test_gemm[plain-129x257x33-b1-Boff1-T] (4-byte loads)
  [B] bsc_gemm.hip gemm_f32_stream_kernel: c_vec / e_vec  gemm_f32_stream_kernel <- test_gemm[epilogue-256x384x160-b1-CT]
                                                        the same kernel, scalar store <- test_gemm[epilogue-256x384x160-b1-Coff1-ld+1-T]
  [B] bsc_gemm.hip gemm_store_tile: vec_e               gemm_f32_mfma_kernel <- test_gemm[epilogue-129x257x33-b1-ctl]
                                                        the same kernel, scalar E <- test_gemm[epilogue-129x257x33-b1-Eoff1]
  [B] bsc_gemm.hip gemm_stream: s.sym (same pointer)    gemm_f32_stream_kernel with s.sym <- test_gemm[plain-256x256x160-b1-same-ctl]; the stream
                                                        kernel also runs without sym, so only the fall-back is a trace fact:
                                                        gemm_f32_mfma_kernel <- test_gemm[plain-256x256x160-b1-same-Aoff1-ld+1]
  [B] bsc_gemm.hip gemv_kcontig_kernel: vec             gemv_kcontig_kernel <- test_gemv[N1-100000x256-ctl]
                                                        the same kernel, 4-byte loads <- test_gemv[N1-100000x256-Moff1]
  [K] bsc_gemm.hip gemm_matvec: vec4                    gemv_mcontig4_kernel <- test_gemv[M1-100000x256-ctl]
                                                        gemv_mcontig_kernel <- test_gemv[M1-100000x256-Mld+1]
  [K] bsc_skinny.hip bsc_gemm_skinny: NT conditions     gemm_skinny_nt_kernel <- test_skinny[nt-ctl], test_skinny[nt_swapped-ctl]
                                                        gemm_f32_* <- test_skinny[nt-big:off1], test_skinny[nt-ctl-skinny0]
  [K] bsc_skinny.hip bsc_gemm_skinny: TN, alignment     gemm_skinny_tn_kernel <- test_skinny[tn-ctl], test_skinny[tn_swapped-ctl]
                                                        gemm_f32_* <- test_skinny[tn-big:ld+1], test_skinny[tn-ctl-skinny0]
  [K] bsc_skinny.hip bsc_gemm_skinny: TN, s * 15 + K    gemm_skinny_tn_kernel <- test_span_gates[skinny-tn-below]
                                                        gemm_f32_* <- test_span_gates[skinny-tn-above]
  [-] bsc_skinny.hip small_span (ld < 2^26)             the ld < 2^26 limit itself stays UNCROSSED: the NT routes need >= 4096 rows at that
                                                        stride (1 TiB), and for TN the s * 15 + K limit above binds first (s < 2^29 / 15).
                                                        Spans past 2^32 bytes BELOW it: test_span_routes_gpu.py test_below_gate[skinny-nt],
                                                        [skinny-nt-swapped] (4100 rows, ld 327 680) and [skinny-tn] (K = 16 384, sb_k = 81 920)
  [K] bsc_fused.hip map_flat                            map_flat_f32_kernel <- test_map_family[map-64x64-ctl]
                                                        map_rows_f32_kernel / map_dense_f32_kernel (map_rows2d, map_is_dense) <-
                                                        test_map_family[map-64x64-ctl-flat0]; map_small_f32_kernel (map_small) <-
                                                        test_map_family[map-64x64-x:off1]
                                                        (map_strided: float64 or > 2^20 outputs only, not reached here)
  [K] bsc_fused.hip short_rows                          map_reduce_rows_f32_kernel <- test_map_family[rowsum-4096x7-ctl]
                                                        map_reduce_wave_kernel <- test_map_family[rowsum-4096x7-x:off1]
  [K] bsc_fused.hip reduce_plan: dense_wave             map_reduce_wave_dense_f32_kernel <- test_map_family[rowsum-4096x64-ctl]
                                                        map_reduce_wave_kernel <- test_map_family[rowsum-4096x64-x:ld+1]
  [K] bsc_fused.hip reduce_plan: dense_lane             map_reduce_lane_dense_f32_kernel <- test_map_family[colsum-64x4096-ctl]
                                                        map_reduce_lane_kernel <- test_map_family[colsum-64x4096-x:off1]
  [K] bsc_tensor.hip bsc_elemwise: dense                elemwise_dense_f32_kernel <- test_map_family[elemwise-64x64-ctl]
                                                        elemwise_kernel <- test_map_family[elemwise-64x64-x:off1]
  [B] bsc_stats.hip normal_stats_partial_kernel: head   normal_stats_partial_kernel <- test_suffstats_normal[off0-n100001] ... [off3-n100001]
  [B] bsc_stats.hip row_sum_kernel(s): 16-byte loads    row_sum_kernel / row_sum_bound_kernel <- test_dirichlet_expectation[7x33-ctl] vs [7x33-off1]
  [K] bsc_stats.hip bsc_softmax_rows: vec4              softmax_rows_vec4_kernel <- test_softmax_rows[4097x64-in:dense-out:dense]
                                                        softmax_rows_small_kernel <- test_softmax_rows[4097x64-in:off1-out:dense];
                                                        softmax_rows_wide_kernel <- test_softmax_rows[31x257-in:dense-out:dense]
  [K] bsc_lda.hip a.vec_c / a.vec_th / lda_stream       lda_sstats_stream_kernel (_k64 / _k32 / _bound likewise) <- test_lda_sstats[K128-V1028-ctl]
                                                        lda_sstats_kernel <- test_lda_sstats[K128-V1028-ctl-stream0], [K128-V1028-c:off1]
                                                        (K = 96 has no stream kernel: lda_sstats_kernel always)
  [B] bsc_lda.hip csc: a.vec_th / csc_fast              lda_sstats_csc_kernel <- test_lda_sstats_csc[K64-ctl] (a.fast) vs [K64-th:off1], [K64-th:ld+1],
                                                        [K64-ctl-fast0] (general loads)
  [-] bsc_mog.hip bsc_mog_estep (no ALIGNMENT gate:     mog_estep_kernel, every layout.  Its gate on the span, ldx < 2^25 (the 32-bit lane
      4-byte loads)                                     offsets of a 32-row tile), is crossed in test_span_routes_gpu.py: test_below_gate[mog-D16],
                                                        [mog-D5], [mog-bx-D16] at 2^25 - 4, test_refused[mog] at 2^25
"""
import ctypes

import numpy as np
import numpy.testing as npt
import pytest

from oracle import svi

import _views as V
from _views import Layout

pytestmark = pytest.mark.gpu

D0 = Layout()
F32, F64 = np.float32, np.float64


def _lay(tag, lay):
    return "" if lay.dense else "%s%s" % (tag, lay.describe())


def case_id(c):
    return c["id"]


def _rs(c):
    return np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(c["id"])) % (2 ** 31))


# =====================================================================================================
# GEMM: bsc_gemm_strided_batched / bsc_gemm_epilogue / bsc_gemm_fused
# A logical [b, M, K]: plain layout = k-contiguous, transpose = m-contiguous.  B logical [b, K, N]: plain =
# n-contiguous, transpose = k-contiguous.  C logical [b, M, N]: plain = sc_n == 1, transpose = sc_m == 1.
# =====================================================================================================
FULL, RAGGED = (256, 384, 160), (129, 257, 33)


def gemm_case(entry, shape, batch=1, a=D0, b=D0, c=D0, e=None, same=False):
    parts = [entry, "%dx%dx%d" % shape, "b%d" % batch] + (["same"] if same else [])
    lays = [_lay("A", a), _lay("B", b), _lay("C", c)]
    lays += [("E" + (e if isinstance(e, str) else e.describe())) if e is not None and entry == "epilogue" and
             not (isinstance(e, Layout) and e.dense) else ""]
    lays = [s for s in lays if s]
    if entry == "epilogue" and e is None:
        lays.append("noE")
    parts += lays or ["ctl"]
    return dict(id="-".join(parts), entry=entry, shape=shape, batch=batch, a=a, b=b, c=c, e=e, same=same)


def _gemm_table():
    t = []
    T = Layout(transpose=True)
    for entry in ("plain", "epilogue", "fused"):
        e = D0 if entry == "epilogue" else None
        for shape in (FULL, RAGGED):
            for batch in (1, 3):
                t.append(gemm_case(entry, shape, batch, e=e))                                   # controls
        # operand orientation, all four
        t.append(gemm_case(entry, FULL, 1, a=T, b=T, e=e))
        t.append(gemm_case(entry, RAGGED, 3, a=T, e=e))
        t.append(gemm_case(entry, RAGGED, 1, b=T, e=e))
        # base offsets and stride remainders, one operand at a time and together
        for k in (1, 2, 3):
            t.append(gemm_case(entry, FULL, 1, a=Layout(base_off=k), e=e))
            t.append(gemm_case(entry, RAGGED, 1, b=Layout(base_off=k, transpose=True), e=e))
            t.append(gemm_case(entry, FULL, 1, a=Layout(ld_extra=k), b=Layout(ld_extra=4 - k, transpose=True), e=e))
            t.append(gemm_case(entry, RAGGED, 3, a=Layout(ld_extra=k, transpose=True), b=Layout(batch_rem=k), e=e))
            t.append(gemm_case(entry, FULL, 3, a=Layout(batch_rem=k), b=Layout(base_off=k, ld_extra=k), e=e))
        t.append(gemm_case(entry, RAGGED, 1, a=Layout(inner=2), b=Layout(inner=2, ld_extra=1), e=e))
        t.append(gemm_case(entry, FULL, 1, a=Layout(inner=2, transpose=True), e=e))
        # aligned views with room between rows: still the 16-byte routes
        t.append(gemm_case(entry, FULL, 3, a=Layout(ld_extra=4), b=Layout(ld_extra=4, transpose=True), e=e))
        t.append(gemm_case(entry, FULL, 1, a=T, b=Layout(ld_extra=4), e=e))
        # the output as a view
        t.append(gemm_case(entry, FULL, 1, c=T, e=e))
        t.append(gemm_case(entry, FULL, 1, c=Layout(base_off=1, ld_extra=1, transpose=True), e=e))
        t.append(gemm_case(entry, RAGGED, 3, c=Layout(base_off=3, ld_extra=3, batch_rem=1), e=e))
        t.append(gemm_case(entry, RAGGED, 1, c=Layout(base_off=2, ld_extra=1, transpose=True), e=e))
        t.append(gemm_case(entry, FULL, 1, c=Layout(ld_extra=5), e=e))
    # the epilogue factor
    for shape in (FULL, RAGGED):
        t.append(gemm_case("epilogue", shape, 1, e=Layout(base_off=1)))
        t.append(gemm_case("epilogue", shape, 1, e=Layout(ld_extra=3)))
        t.append(gemm_case("epilogue", shape, 1, e="bcast"))
        t.append(gemm_case("epilogue", shape, 1, c=T, e=Layout(transpose=True)))
        t.append(gemm_case("epilogue", shape, 3, e=Layout(base_off=2, ld_extra=1, batch_rem=3)))
    # X^T X with both operands the same pointer
    for entry in ("plain", "epilogue"):
        e = D0 if entry == "epilogue" else None
        t.append(gemm_case(entry, (256, 256, 160), 1, same=True, e=e))
        t.append(gemm_case(entry, (256, 256, 160), 1, a=Layout(base_off=1, ld_extra=1), same=True, e=e))
        t.append(gemm_case(entry, (132, 132, 1000), 1, a=Layout(ld_extra=4), same=True, e=e))
        t.append(gemm_case(entry, (129, 129, 33), 1, a=Layout(base_off=3), same=True, e=e))
    return t


def _rem(x):
    return x % 4


def gemm_axes(c):
    M, N, K = c["shape"]
    sa = c["a"].geometry((c["batch"], M, K))[1]
    sb = c["b"].geometry((c["batch"], K, N))[1]
    sc = c["c"].geometry((c["batch"], M, N))[1]
    e = c["e"]
    e_kind = "none" if e is None else e if isinstance(e, str) else \
        "dense" if e.dense else "misaligned" if e.base_off else "odd" if max(e.geometry((M, N))[1]) % 2 else "view"
    lays = [c["a"], c["b"], c["c"]] + ([e] if isinstance(e, Layout) else [])
    return dict(
        entry=c["entry"], shape=c["shape"], batch=c["batch"],
        a_contig="m" if c["a"].transpose else "k", b_contig="k" if c["b"].transpose else "n",
        c_contig="m" if c["c"].transpose else "n",
        in_base_off={c["a"].base_off, c["b"].base_off},
        in_ld_rem={_rem(max(sa[1:])), _rem(max(sb[1:]))},
        in_batch_rem={_rem(sa[0]), _rem(sb[0])} if c["batch"] > 1 else {0},
        m_rem=_rem(M) != 0, n_rem=_rem(N) != 0, k_rem=_rem(K) != 0,
        inner2=c["a"].inner == 2 or c["b"].inner == 2,
        c_odd_ld=max(sc[1:]) % 2 == 1, c_base_off=c["c"].base_off,
        e=e_kind, same=c["same"],
        control=all(l.dense for l in lays) and not c["same"] and e != "bcast")


GEMM_REQUIRED = dict(
    entry=["plain", "epilogue", "fused"], shape=[FULL, RAGGED], batch=[1, 3], a_contig=["k", "m"], b_contig=["k", "n"],
    c_contig=["m", "n"], in_base_off=[1, 2, 3], in_ld_rem=[0, 1, 2, 3], in_batch_rem=[1, 2, 3], m_rem=[False, True],
    n_rem=[False, True], k_rem=[False, True], inner2=[True], c_odd_ld=[True], c_base_off=[1, 2, 3],
    e=["dense", "misaligned", "odd", "bcast"], same=[True])


def gemm_data(c):
    M, N, K = c["shape"]
    rs, nb = _rs(c), c["batch"]
    lead = (nb,) if nb > 1 else ()
    pos = c["entry"] == "epilogue"                         # C / dot(..) needs a product away from zero
    draw = (lambda s: (rs.rand(*s) + 0.1)) if pos else (lambda s: rs.standard_normal(s))
    if c["same"]:
        X = draw((K, M)).astype(F32)
        A, B = X.T, X
    else:
        A, B = draw(lead + (M, K)).astype(F32), draw(lead + (K, N)).astype(F32)
    E = None
    if c["entry"] == "epilogue" and c["e"] is not None:
        E = (rs.rand(N) + 0.5).astype(F32) if c["e"] == "bcast" else (rs.rand(*(lead + (M, N))) + 0.5).astype(F32)
    return A, B, E


def gemm_power(c):
    return -1 if c["entry"] == "epilogue" and (c["a"].base_off + c["shape"][2]) % 2 else 1


def gemm_reference(c):
    A, B, E = gemm_data(c)
    A64, B64 = A.astype(F64), B.astype(F64)
    if c["entry"] == "fused":
        A64, B64 = A64 * A64, np.abs(B64)
    P = A64 @ B64
    bound = np.abs(A64) @ np.abs(B64)
    if c["entry"] == "epilogue":
        P = 2.5 * P ** gemm_power(c) * (1.0 if E is None else E.astype(F64))
    return dict(C=P, bound=bound)


def gemm_fused_expected(c):
    """Whether bsc_gemm_fused applies the producers (*handled = 1): only the persistent LDS-DMA kernel does, and
    it takes an operand (csrc/bsc_gemm.hip dma_ok) when the base is 16-byte aligned, the batch stride a multiple
    of 4 and EITHER its free axis is contiguous with an extent % 4 == 0 and a contraction stride % 4 == 0, OR the
    contraction axis is contiguous with K % 4 == 0 and a free-axis stride % 4 == 0 (the spans here are far
    below 2^31).  From the documented conditions, not from what the library answers."""
    M, N, K = c["shape"]
    nb = c["batch"]

    def ok(lay, shape, ext_mn, mn_axis):
        st = lay.geometry(shape)[1]
        s_b = st[0] if nb > 1 else 0
        s_mn, s_k = (st[-2], st[-1]) if mn_axis == 0 else (st[-1], st[-2])
        if lay.base_off or s_b % 4:
            return False
        if s_mn == 1:
            return ext_mn % 4 == 0 and s_k % 4 == 0
        return s_k == 1 and K % 4 == 0 and s_mn % 4 == 0

    lead = (nb,) if nb > 1 else ()
    return ok(c["a"], lead + (M, K), M, 0) and ok(c["b"], lead + (K, N), N, 1)


def _bs(view):
    return (0,) + view.strides if len(view.strides) == 2 else view.strides


# =====================================================================================================
# the skinny routes and GEMV, through bsc_gemm_strided_batched
# =====================================================================================================
def skinny_case(kind, big=D0, K=None, skinny=1):
    K = K if K is not None else (64 if kind.startswith("nt") else 20000)
    tag = [kind] + ([_lay("big:", big)] if not big.dense else []) + (["K%d" % K] if K % 4 else [])
    tag += ["ctl"] if big.dense and K % 4 == 0 else []
    tag += ["skinny0"] if not skinny else []
    return dict(id="-".join(tag), kind=kind, big=big, K=K, skinny=skinny)


def _skinny_table():
    t = []
    for kind in ("nt", "nt_swapped", "tn", "tn_swapped"):
        t += [skinny_case(kind), skinny_case(kind, skinny=0), skinny_case(kind, Layout(base_off=1)),
              skinny_case(kind, Layout(base_off=2)), skinny_case(kind, Layout(ld_extra=1)),
              skinny_case(kind, Layout(base_off=3, ld_extra=3)), skinny_case(kind, Layout(ld_extra=4)),
              skinny_case(kind, K=62 if kind.startswith("nt") else 20001)]
    return t


def skinny_shapes(c):
    """-> (M, N, K, layout of A, layout of B): the large operand carries c['big'] on top of its orientation."""
    big, K, T = c["big"], c["K"], Layout(transpose=True)
    bigT = Layout(big.base_off, big.ld_extra, True, big.inner, big.batch_rem)
    if c["kind"] == "nt":               # B [K, N] with k-contiguous rows n
        return 8, 4100, K, D0, bigT
    if c["kind"] == "nt_swapped":       # A [M, K] long, k-contiguous
        return 4100, 8, K, big, T
    if c["kind"] == "tn":               # A [M, K] k-contiguous (small M), B [K, N] n-contiguous, long K
        return 8, 64, K, D0, big
    return 64, 8, K, bigT, T            # tn_swapped: A m-contiguous [M, K], B k-contiguous


def skinny_axes(c):
    return dict(kind=c["kind"], big_base_off=c["big"].base_off, big_odd_ld=c["big"].ld_extra % 2 == 1,
                k_rem=c["K"] % 4 != 0, skinny=c["skinny"], control=c["big"].dense and c["K"] % 4 == 0 and c["skinny"] == 1)


SKINNY_REQUIRED = dict(kind=["nt", "nt_swapped", "tn", "tn_swapped"], big_base_off=[0, 1, 2, 3], big_odd_ld=[True],
                       k_rem=[True], skinny=[0, 1])


def skinny_data(c):
    M, N, K, la, lb = skinny_shapes(c)
    rs = _rs(c)
    return rs.standard_normal((M, K)).astype(F32), rs.standard_normal((K, N)).astype(F32)


def gemv_case(side, shape, mat=D0, x=D0, y=D0):
    tag = [side, "%dx%d" % shape, _lay("M", mat), _lay("x", x), _lay("y", y)]
    tag = [s for s in tag if s]
    return dict(id="-".join(tag + (["ctl"] if mat.dense and x.dense and y.dense else [])), side=side, shape=shape,
                mat=mat, x=x, y=y)


def _gemv_table():
    t = []
    T = Layout(transpose=True)
    for side in ("N1", "M1"):
        for shape in ((100000, 256), (4097, 33)):
            big = shape[0] > 50000
            t.append(gemv_case(side, shape))
            t.append(gemv_case(side, shape, mat=Layout(base_off=1)))
            t.append(gemv_case(side, shape, mat=Layout(ld_extra=1)))
            if not big:
                t.append(gemv_case(side, shape, mat=T))
                t.append(gemv_case(side, shape, mat=Layout(base_off=2, ld_extra=3, transpose=True)))
                for k in (1, 2, 3):
                    t.append(gemv_case(side, shape, x=Layout(base_off=k)))
                t.append(gemv_case(side, shape, x=Layout(inner=2)))
                t.append(gemv_case(side, shape, mat=Layout(base_off=3), x=Layout(base_off=1, inner=2), y=Layout(base_off=1)))
                t.append(gemv_case(side, shape, y=Layout(inner=2)))
    t.append(gemv_case("N1", (100000, 256), x=Layout(base_off=1)))
    t.append(gemv_case("M1", (100000, 256), x=Layout(inner=2)))
    return t


def gemv_axes(c):
    return dict(side=c["side"], shape=c["shape"], mat_base_off=c["mat"].base_off, mat_odd_ld=c["mat"].ld_extra % 2 == 1,
                x_base_off=c["x"].base_off, x_inner=c["x"].inner, control=c["mat"].dense and c["x"].dense and c["y"].dense)


GEMV_REQUIRED = dict(side=["N1", "M1"], shape=[(100000, 256), (4097, 33)], mat_base_off=[0, 1], mat_odd_ld=[True],
                     x_base_off=[1, 2, 3], x_inner=[2])


def gemv_data(c):
    rows, cols = c["shape"]
    rs = _rs(c)
    mat = rs.standard_normal((rows, cols)).astype(F32)
    x = rs.standard_normal(cols if c["side"] == "N1" else rows).astype(F32)
    return mat, x


# =====================================================================================================
# bsc_softmax_rows, the Dirichlet expectations, the float32 natural-gradient step, bsc_suffstats_normal
# =====================================================================================================
def softmax_case(rows, cols, lin=D0, lout=D0):
    return dict(id="%dx%d-in:%s-out:%s" % (rows, cols, lin.describe(), lout.describe()), rows=rows, cols=cols,
                lin=lin, lout=lout)


def _softmax_table():
    t = []
    for cols in (8, 12, 63, 64, 256, 257):
        for rows in (1, 31, 4097):
            t.append(softmax_case(rows, cols))
        for k in (1, 2, 3):
            t.append(softmax_case(31, cols, Layout(base_off=k), Layout(ld_extra=k)))
            t.append(softmax_case(4097 if cols <= 64 else 31, cols, Layout(ld_extra=k), Layout(base_off=k)))
        t.append(softmax_case(31, cols, Layout(ld_extra=4), Layout(ld_extra=4)))
        t.append(softmax_case(4097 if cols == 64 else 1, cols, Layout(base_off=1), D0))
        t.append(softmax_case(31, cols, D0, Layout(base_off=2, ld_extra=5)))
    return t


def softmax_axes(c):
    return dict(cols=c["cols"], rows=c["rows"], ld_in_rem=_rem(c["cols"] + c["lin"].ld_extra),
                ld_out_rem=_rem(c["cols"] + c["lout"].ld_extra), base_in=c["lin"].base_off, base_out=c["lout"].base_off,
                control=c["lin"].dense and c["lout"].dense)


SOFTMAX_REQUIRED = dict(cols=[8, 12, 63, 64, 256, 257], rows=[1, 31, 4097], ld_in_rem=[0, 1, 2, 3],
                        ld_out_rem=[0, 1, 2, 3], base_in=[0, 1, 2, 3], base_out=[0, 1, 2, 3])


def softmax_data(c):
    rs = _rs(c)
    x = (rs.standard_normal((c["rows"], c["cols"])) * 6.0).astype(F32)
    x[0, 0] = 80.0
    x[-1, -1] = -90.0
    return x


def dirichlet_case(entry, rows, cols, lay=D0):
    return dict(id="%s%dx%d-%s" % ("" if entry == "dirichlet" else "bound-", rows, cols, "ctl" if lay.dense else lay.describe()),
                entry=entry, rows=rows, cols=cols, lay=lay)


def _dirichlet_table(entry):
    t = []
    for rows, cols in ((7, 33), (128, 5000), (300, 16), (5, 4098)):
        t.append(dirichlet_case(entry, rows, cols))
        for k in (1, 2, 3):
            t.append(dirichlet_case(entry, rows, cols, Layout(base_off=k)))
            t.append(dirichlet_case(entry, rows, cols, Layout(ld_extra=k)))
        t.append(dirichlet_case(entry, rows, cols, Layout(base_off=2, ld_extra=4)))
        t.append(dirichlet_case(entry, rows, cols, Layout(ld_extra=4)))
    return t


def dirichlet_axes(c):
    return dict(ld_rem=_rem(c["cols"] + c["lay"].ld_extra), base_off=c["lay"].base_off, cols_rem=_rem(c["cols"]) != 0,
                control=c["lay"].dense)


DIRICHLET_REQUIRED = dict(ld_rem=[0, 1, 2, 3], base_off=[0, 1, 2, 3], cols_rem=[False, True])


def dirichlet_data(c):
    return _rs(c).gamma(1.0, 2.0, (c["rows"], c["cols"])).astype(F32) + F32(1e-3)


def natgrad_case(rows, cols, leta=D0, lmsg=D0):
    return dict(id="%dx%d-eta:%s-msg:%s" % (rows, cols, leta.describe(), lmsg.describe()), rows=rows, cols=cols,
                leta=leta, lmsg=lmsg)


def _natgrad_table():
    t = []
    for rows, cols in ((64, 1028), (33, 1001)):
        t.append(natgrad_case(rows, cols))
        for k in (1, 2, 3):
            t.append(natgrad_case(rows, cols, Layout(base_off=k, ld_extra=k), Layout(ld_extra=4 - k)))
            t.append(natgrad_case(rows, cols, Layout(ld_extra=4 - k), Layout(base_off=k, ld_extra=k)))
    return t


def natgrad_axes(c):
    return dict(ld_rem={_rem(c["cols"] + c["leta"].ld_extra), _rem(c["cols"] + c["lmsg"].ld_extra)},
                base_off={c["leta"].base_off, c["lmsg"].base_off}, cols_rem=_rem(c["cols"]) != 0,
                control=c["leta"].dense and c["lmsg"].dense)


def natgrad_data(c):
    rs = _rs(c)
    return (rs.rand(c["rows"], c["cols"]) + 0.5).astype(F32), (rs.rand(c["rows"], c["cols"]) * 3.0).astype(F32)


def suffstats_case(off, n):
    return dict(id="off%d-n%d" % (off, n), off=off, n=n)


def suffstats_axes(c):
    return dict(off=c["off"], n=c["n"], control=c["off"] == 0)


def suffstats_data(c):
    return (_rs(c).standard_normal(c["n"]) * 3.0 + 1.0).astype(F32)


# =====================================================================================================
# the LDA statistic (dense and sparse counts) and the mixture E-step
# =====================================================================================================
def lda_case(K, V, bound=False, c=D0, th=D0, bt=D0, o=D0, stream=1):
    lays = [s for s in (_lay("c:", c), _lay("th:", th), _lay("bt:", bt), _lay("o:", o)) if s]
    tag = ["bound"] * bound + ["K%d" % K, "V%d" % V] + (lays or ["ctl"]) + (["stream0"] if not stream else [])
    return dict(id="-".join(tag), K=K, V=V, bound=bound, c=c, th=th, bt=bt, o=o, stream=stream, docs=300)


def _lda_table(bound):
    t = []
    for K in (32, 64, 96, 128):
        for V in (1028, 1029):
            t.append(lda_case(K, V, bound))
        t.append(lda_case(K, 1028, bound, stream=0))
        k = (K // 32 - 1) % 3 + 1
        t.append(lda_case(K, 1028, bound, c=Layout(base_off=k)))
        t.append(lda_case(K, 1028, bound, c=Layout(ld_extra=k)))
        t.append(lda_case(K, 1028, bound, th=Layout(base_off=k)))
        t.append(lda_case(K, 1028, bound, th=Layout(ld_extra=k)))
        t.append(lda_case(K, 1029, bound, bt=Layout(base_off=k, ld_extra=k)))
        t.append(lda_case(K, 1028, bound, o=Layout(base_off=k)))
        t.append(lda_case(K, 1028, bound, o=Layout(ld_extra=k)))
        t.append(lda_case(K, 1029, bound, c=Layout(base_off=1, ld_extra=2), th=Layout(base_off=3, ld_extra=1),
                          bt=Layout(base_off=2, ld_extra=2), o=Layout(base_off=1, ld_extra=3)))
    return t


def lda_axes(c):
    four = (c["c"], c["th"], c["bt"], c["o"])
    return dict(K=c["K"], v_rem=c["V"] % 4, c_view=(c["c"].base_off > 0, c["c"].ld_extra % 4 > 0),
                th_view=(c["th"].base_off > 0, c["th"].ld_extra % 4 > 0), bt_view=(c["bt"].base_off > 0, c["bt"].ld_extra % 4 > 0),
                o_view=(c["o"].base_off > 0, c["o"].ld_extra % 4 > 0), stream=c["stream"] if all(l.dense for l in four) else None,
                control=all(l.dense for l in four) and c["stream"] == 1)


_VIEWS = [(True, False), (False, True)]
LDA_REQUIRED = dict(K=[32, 64, 96, 128], v_rem=[0, 1], c_view=_VIEWS, th_view=_VIEWS, o_view=_VIEWS, bt_view=[(True, True)],
                    stream=[0, 1])


def lda_data(c, density=None):
    rs = _rs(c)
    docs, V, K = c["docs"], c["V"], c["K"]
    C = rs.poisson(0.3, (docs, V)).astype(F32)
    if density is not None:
        C = C * (rs.uniform(size=(docs, V)) < density)
    Th = rs.uniform(0.1, 1.0, (docs, K)).astype(F32)
    Bt = rs.uniform(0.1, 1.0, (K, V)).astype(F32)
    return C.astype(F32), Th, Bt


def csc_case(K, bound=False, th=D0, fast=1):
    tag = ["bound"] * bound + ["K%d" % K, "ctl" if th.dense else "th:" + th.describe()] + (["fast0"] if not fast else [])
    return dict(id="-".join(tag), K=K, V=501, docs=333, bound=bound, th=th, fast=fast)


def _csc_table(bound):
    t = []
    for K in (32, 64, 96, 128):
        t += [csc_case(K, bound), csc_case(K, bound, fast=0)]
        for k in (1, 2, 3):
            for fast in (0, 1):
                t.append(csc_case(K, bound, Layout(base_off=k), fast=fast))
                t.append(csc_case(K, bound, Layout(ld_extra=k), fast=fast))
    return t


def csc_axes(c):
    return dict(th_base_off=c["th"].base_off, th_odd_ld=c["th"].ld_extra % 2 == 1, fast=c["fast"],
                view_and_fast=(c["th"].base_off, c["th"].ld_extra % 4, c["fast"]), control=c["th"].dense and c["fast"] == 1)


CSC_REQUIRED = dict(th_base_off=[0, 1, 2, 3], th_odd_ld=[True], fast=[0, 1],
                    view_and_fast=[(b, 0, f) for b in (1, 2, 3) for f in (0, 1)] + [(0, e, f) for e in (1, 2, 3) for f in (0, 1)])


def mog_case(D, lay=D0):
    return dict(id="D%d-%s" % (D, "ctl" if lay.dense else lay.describe()), D=D, lay=lay, N=5001, K=5)


def _mog_table():
    t = []
    for D in (1, 3, 16):
        t.append(mog_case(D))
        for k in (1, 2, 3):
            t.append(mog_case(D, Layout(base_off=k)))
            t.append(mog_case(D, Layout(ld_extra=k)))          # ldx = D + k: every remainder for every D below
            t.append(mog_case(D, Layout(base_off=4 - k, ld_extra=k + 1 if k < 3 else 5)))
    return t


def mog_axes(c):
    return dict(base_off=c["lay"].base_off, ldx_rem=_rem(c["D"] + c["lay"].ld_extra), D=c["D"], control=c["lay"].dense)


MOG_REQUIRED = dict(base_off=[1, 2, 3], ldx_rem=[1, 2, 3], D=[1, 3, 16])


def mog_data(c):
    rs = _rs(c)
    N, D, K = c["N"], c["D"], c["K"]
    cen = rs.standard_normal((K, D)) * 2
    X = (cen[rs.randint(K, size=N)] + rs.standard_normal((N, D))).astype(F32)
    T = rs.uniform(0.5, 2.0, (K, D))
    Wmat = np.concatenate([T * cen, -0.5 * T], axis=1).astype(F32)
    cvec = (-0.5 * (T * cen ** 2).sum(1)).astype(F32)
    return X, Wmat, cvec


# =====================================================================================================
# bsc_map_reduce / bsc_sum / bsc_elemwise / bsc_convert
# value(r, c) = 0.5 * (x[r, c] + y[r, c]) + 0.25 (map_reduce), x + y (elemwise), x (sum, convert); every value > 0
# =====================================================================================================
Y_KINDS = ("dense", "rowvec", "percol", "scalar", "diag", "transposed", "offset", "oddld")


def map_case(op, shape, x=D0, y="dense", out=D0, flat=1):
    tag = [op, "%dx%d" % shape] + [s for s in (_lay("x:", x), "" if y == "dense" else "y:" + y, _lay("o:", out)) if s]
    ctl = x.dense and y == "dense" and out.dense
    return dict(id="-".join(tag + (["ctl"] if ctl else []) + (["flat0"] if not flat else [])), op=op, shape=shape, x=x, y=y,
                out=out, flat=flat)


def _map_table():
    t = []
    shapes = {"map": [(64, 64), (64, 66), (4100, 4)], "elemwise": [(64, 64), (64, 66)], "convert": [(64, 64), (64, 66)],
              "rowsum": [(4096, 64), (4096, 7), (4097, 1030)], "colsum": [(64, 4096), (1030, 4097)],
              "sum": [(4096, 64), (4097, 1030), (64, 4096)]}
    for op, shs in shapes.items():
        for sh in shs:
            t.append(map_case(op, sh))
            if op == "map":
                t.append(map_case(op, sh, flat=0))
            for lay in (Layout(base_off=1), Layout(base_off=2), Layout(base_off=3), Layout(ld_extra=1), Layout(ld_extra=3),
                        Layout(transpose=True), Layout(ld_extra=4)):
                t.append(map_case(op, sh, x=lay))
            if op in ("map", "elemwise", "rowsum", "colsum"):
                for y in Y_KINDS[1:]:
                    if y == "diag" and op in ("rowsum", "colsum"):
                        continue
                    t.append(map_case(op, sh, y=y))
            if op in ("map", "elemwise", "convert"):
                for lay in (Layout(base_off=1), Layout(ld_extra=1), Layout(base_off=2, ld_extra=3)):
                    t.append(map_case(op, sh, out=lay))
            elif op in ("rowsum", "colsum"):
                t.append(map_case(op, sh, out=Layout(base_off=1)))
                t.append(map_case(op, sh, out=Layout(inner=2)))
    return t


def map_axes(c):
    n_out = c["shape"][0] * c["shape"][1] if c["op"] in ("map", "elemwise", "convert") else \
        c["shape"][0] if c["op"] in ("rowsum", "sum") else c["shape"][1]
    return dict(op=c["op"], y=c["y"], x_base_off=c["x"].base_off, x_odd_ld=c["x"].ld_extra % 2 == 1, x_T=c["x"].transpose,
                out_view=("offset" if c["out"].base_off else "oddld" if c["out"].ld_extra % 2 or c["out"].inner == 2 else "dense"),
                row_rem=_rem(c["shape"][1]) != 0, big=n_out >= 4096, flat=c["flat"],
                control=c["x"].dense and c["y"] == "dense" and c["out"].dense and c["flat"] == 1)


MAP_REQUIRED = dict(op=["map", "elemwise", "convert", "rowsum", "colsum", "sum"], y=list(Y_KINDS), x_base_off=[0, 1, 2, 3],
                    x_odd_ld=[True], x_T=[True], out_view=["dense", "offset", "oddld"], row_rem=[False, True], big=[True],
                    flat=[0, 1])


def map_data(c):
    rs = _rs(c)
    R, C = c["shape"]
    x = (rs.rand(R, C) + 0.25).astype(F32)
    y = c["y"]
    if y in ("dense", "transposed", "offset", "oddld"):
        yv = (rs.rand(R, C) + 0.25).astype(F32)
    elif y == "rowvec":
        yv = (rs.rand(C) + 0.25).astype(F32)
    elif y == "percol":
        yv = (rs.rand(R) + 0.25).astype(F32)
    elif y == "scalar":
        yv = (rs.rand(1) + 0.25).astype(F32)
    else:                                                   # the diagonal of a square matrix, one value per row
        yv = (rs.rand(R, R) + 0.25).astype(F32)
    return x, yv


def map_y_full(c, yv):
    R, C = c["shape"]
    y = c["y"]
    if y == "rowvec":
        return np.broadcast_to(yv[None, :], (R, C))
    if y == "percol":
        return np.broadcast_to(yv[:, None], (R, C))
    if y == "scalar":
        return np.broadcast_to(yv.reshape(1, 1), (R, C))
    if y == "diag":
        return np.broadcast_to(np.diagonal(yv)[:, None], (R, C))
    return yv


def map_reference(c):
    x, yv = map_data(c)
    x64, y64 = x.astype(F64), map_y_full(c, yv).astype(F64)
    op = c["op"]
    if op == "map":
        return dict(out=0.5 * (x64 + y64) + 0.25)
    if op == "elemwise":
        return dict(out=x64 + y64)
    if op == "convert":
        return dict(out=x64)
    if op == "sum":
        return dict(out=x64.sum(1))
    v = 0.5 * (x64 + y64) + 0.25
    return dict(out=v.sum(1) if op == "rowsum" else v.sum(0))


# =====================================================================================================
# the tables, what each must visit (tests/test_views_cpu.py checks it), and every reference on the host
# =====================================================================================================
TABLES = {
    "gemm": _gemm_table(), "skinny": _skinny_table(), "gemv": _gemv_table(), "softmax": _softmax_table(),
    "dirichlet": _dirichlet_table("dirichlet"), "dirichlet_bound": _dirichlet_table("dirichlet_bound"),
    "natgrad_2d": _natgrad_table(),
    "suffstats": [suffstats_case(o, n) for o in range(4) for n in (0, 1, 2, 3, 4, 5, 1023, 100001)],
    "lda": _lda_table(False), "lda_bound": _lda_table(True), "lda_csc": _csc_table(False), "lda_csc_bound": _csc_table(True),
    "mog": _mog_table(), "map": _map_table(),
}
REQUIRED = {
    "gemm": GEMM_REQUIRED, "skinny": SKINNY_REQUIRED, "gemv": GEMV_REQUIRED, "softmax": SOFTMAX_REQUIRED,
    "dirichlet": DIRICHLET_REQUIRED, "dirichlet_bound": DIRICHLET_REQUIRED,
    "natgrad_2d": dict(ld_rem=[0, 1, 2, 3], base_off=[0, 1, 2, 3], cols_rem=[False, True]),
    "suffstats": dict(off=[0, 1, 2, 3], n=[0, 1, 2, 3, 4, 5, 1023, 100001]),
    "lda": LDA_REQUIRED, "lda_bound": LDA_REQUIRED, "lda_csc": CSC_REQUIRED, "lda_csc_bound": CSC_REQUIRED,
    "mog": MOG_REQUIRED, "map": MAP_REQUIRED,
}
_AXES = {"gemm": gemm_axes, "skinny": skinny_axes, "gemv": gemv_axes, "softmax": softmax_axes, "dirichlet": dirichlet_axes,
         "dirichlet_bound": dirichlet_axes, "natgrad_2d": natgrad_axes, "suffstats": suffstats_axes, "lda": lda_axes,
         "lda_bound": lda_axes, "lda_csc": csc_axes, "lda_csc_bound": csc_axes, "mog": mog_axes, "map": map_axes}


def axes_of(entry, c):
    return _AXES[entry](c)


def _softmax_reference(c):
    x64 = softmax_data(c).astype(F64)
    m = x64.max(1, keepdims=True)
    w = np.exp(x64 - m)
    return dict(out=w / w.sum(1, keepdims=True), lse=(m + np.log(w.sum(1, keepdims=True)))[:, 0])


def _natgrad_reference(c):
    eta, msg = natgrad_data(c)
    rho, scale, eta0 = F64(F32(0.3)), F64(F32(1.7)), F64(F32(0.01))
    return dict(eta=(1 - rho) * eta.astype(F64) + rho * (eta0 + scale * msg.astype(F64)))


def reference(entry, c):
    """name -> float64 array: what the test of `entry` compares the device result with."""
    if entry == "gemm":
        return gemm_reference(c)
    if entry == "skinny":
        A, B = skinny_data(c)
        return dict(C=A.astype(F64) @ B.astype(F64), bound=np.abs(A.astype(F64)) @ np.abs(B.astype(F64)))
    if entry == "gemv":
        mat, x = gemv_data(c)
        m64, x64 = mat.astype(F64), x.astype(F64)
        return dict(y=m64 @ x64, bound=np.abs(m64) @ np.abs(x64)) if c["side"] == "N1" else \
            dict(y=x64 @ m64, bound=np.abs(x64) @ np.abs(m64))
    if entry == "softmax":
        return _softmax_reference(c)
    if entry in ("dirichlet", "dirichlet_bound"):
        lam = dirichlet_data(c)
        out = dict(out=svi.dirichlet_expectation(lam))
        if entry == "dirichlet_bound":
            out["bound"] = float(svi.dirichlet_neg_kl(lam, 0.01).sum())
        return out
    if entry == "natgrad_2d":
        return _natgrad_reference(c)
    if entry == "suffstats":
        return dict(stats=svi.normal_suffstats(suffstats_data(c)))
    if entry in ("lda", "lda_bound", "lda_csc", "lda_csc_bound"):
        C, Th, Bt = lda_data(c, 0.05 if "csc" in entry else None)
        out = dict(sstats=svi.lda_sstats(C, Th, Bt))
        if entry.endswith("bound"):
            out["ll"] = svi.lda_local_bound(C, Th, Bt)
            out["ll_scale"] = float((C.astype(F64) * np.abs(np.log(Th.astype(F64) @ Bt.astype(F64)))).sum())
        return out
    if entry == "mog":
        X, Wmat, cvec = mog_data(c)
        s, l = svi.mog_local_step(X, Wmat, cvec)
        return dict(stats=s, lse=l)
    if entry == "map":
        return map_reference(c)
    raise KeyError(entry)


def _params(entry):
    return pytest.mark.parametrize("c", TABLES[entry], ids=case_id)


# ---- contexts with one option changed, closed when the module is done --------------------------------
@pytest.fixture(scope="module")
def alt(ctx):
    """alt(name=value) -> a second Context on the session context's device and on torch's current stream (the one
    the session context was created on, so buffers allocated here belong to the stream both launch on)."""
    from bayesic_amd.device import Context
    made = {}

    def get(**options):
        key = tuple(sorted(options.items()))
        if key not in made:
            made[key] = Context(ctx.device_index, stream=ctx.stream, options=options)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _i64(values):
    values = [int(v) for v in values]
    return (ctypes.c_int64 * max(len(values), 1))(*values)


def _f64(t):
    return t.cpu().numpy().astype(F64)


# =====================================================================================================
# the tests
# =====================================================================================================
@_params("gemm")
def test_gemm(ctx, c):
    dev = ctx.device
    M, N, K = c["shape"]
    nb = c["batch"]
    A, B, E = gemm_data(c)
    want = reference("gemm", c)
    if c["same"]:
        x = V.place(np.ascontiguousarray(B), c["a"], dev)              # X [K, M]; A = X^T through the strides
        a_args = (x.ptr, 0, x.strides[1], x.strides[0])
        b_args = (x.ptr, 0, x.strides[0], x.strides[1])
    else:
        a, b = V.place(A, c["a"], dev), V.place(B, c["b"], dev)
        a_args, b_args = (a.ptr,) + _bs(a), (b.ptr,) + _bs(b)
    out = V.out_like(((nb,) if nb > 1 else ()) + (M, N), F32, c["c"], dev)
    c_args = (out.ptr,) + _bs(out)
    dims = (0, nb, M, N, K)
    if c["entry"] == "plain":
        ctx.call("bsc_gemm_strided_batched", *dims, *a_args, *b_args, *c_args)
    elif c["entry"] == "epilogue":
        if E is None:
            e_args = (None, 0, 0, 0)
        elif c["e"] == "bcast":
            ev = V.place(E, D0, dev)
            e_args = (ev.ptr, 0, 0, 1)
        else:
            ev = V.place(E, c["e"], dev)
            e_args = (ev.ptr,) + _bs(ev)
        ctx.call("bsc_gemm_epilogue", *dims, *a_args, *b_args, *c_args, gemm_power(c), 2.5, *e_args)
    else:
        handled = ctypes.c_int32(-1)
        ctx.call("bsc_gemm_fused", *dims, *a_args, 1, *b_args, 3, *c_args, 0, 1.0, None, 0, 0, 0, ctypes.byref(handled))
        ctx.sync()
        assert handled.value == int(gemm_fused_expected(c)), "handled=%d" % handled.value
        if handled.value == 0:                                         # nothing launched: C must be untouched, all of it
            bits = out.buf.view(V._SIGNED[out.np_dtype]).cpu().numpy().view(np.uint32)
            assert (bits == V.SENTINEL[np.dtype(F32)]).all()
            return
    ctx.sync()
    got = _f64(out.t)
    if c["entry"] == "plain":
        err = np.abs(got - want["C"])
        print("max err / bound", float((err / (want["bound"] + 1e-30)).max()))
        assert (err <= 1e-5 * want["bound"] + 1e-30).all()
    elif c["entry"] == "epilogue":
        npt.assert_allclose(got, want["C"], rtol=3e-5)
    else:
        npt.assert_allclose(got, want["C"], rtol=2e-4, atol=2e-5 * np.abs(want["C"]).max())
    out.check_guard()


@_params("skinny")
def test_skinny(ctx, alt, c):
    cx = ctx if c["skinny"] else alt(gemm_skinny=0)
    dev = ctx.device
    M, N, K, la, lb = skinny_shapes(c)
    A, B = skinny_data(c)
    want = reference("skinny", c)
    a, b = V.place(A, la, dev), V.place(B, lb, dev)
    out = V.out_like((M, N), F32, D0, dev)
    cx.call("bsc_gemm_strided_batched", 0, 1, M, N, K, a.ptr, 0, *a.strides, b.ptr, 0, *b.strides, out.ptr, 0, *out.strides)
    cx.sync()
    err = np.abs(_f64(out.t) - want["C"])
    print("max err / bound", float((err / (want["bound"] + 1e-30)).max()))
    assert (err <= 1e-5 * want["bound"] + 1e-30).all()
    out.check_guard()


@_params("gemv")
def test_gemv(ctx, c):
    dev = ctx.device
    rows, cols = c["shape"]
    mat, x = gemv_data(c)
    want = reference("gemv", c)
    m, xv = V.place(mat, c["mat"], dev), V.place(x, c["x"], dev)
    n_out = rows if c["side"] == "N1" else cols
    out = V.out_like((n_out,), F32, c["y"], dev)
    if c["side"] == "N1":                       # [rows, cols] @ [cols, 1]
        ctx.call("bsc_gemm_strided_batched", 0, 1, rows, 1, cols, m.ptr, 0, *m.strides, xv.ptr, 0, xv.strides[0], 1,
                 out.ptr, 0, out.strides[0], 1)
    else:                                       # [1, rows] @ [rows, cols]
        ctx.call("bsc_gemm_strided_batched", 0, 1, 1, cols, rows, xv.ptr, 0, 1, xv.strides[0], m.ptr, 0, *m.strides,
                 out.ptr, 0, 1, out.strides[0])
    ctx.sync()
    err = np.abs(_f64(out.t) - want["y"])
    print("max err / bound", float((err / (want["bound"] + 1e-30)).max()))
    assert (err <= 1e-5 * want["bound"] + 1e-30).all()
    out.check_guard()


@_params("softmax")
def test_softmax_rows(ctx, c):
    dev = ctx.device
    rows, cols = c["rows"], c["cols"]
    xin = V.place(softmax_data(c), c["lin"], dev)
    out = V.out_like((rows, cols), F32, c["lout"], dev)
    lse = V.out_like((rows,), F32, D0, dev)
    ctx.call("bsc_softmax_rows", xin.ptr, rows, cols, xin.strides[0], out.ptr, out.strides[0], lse.ptr)
    ctx.sync()
    want = reference("softmax", c)
    npt.assert_allclose(out.numpy(), want["out"], rtol=3e-5, atol=1e-30)
    npt.assert_allclose(lse.numpy(), want["lse"], rtol=1e-6, atol=1e-6)
    npt.assert_allclose(out.numpy().sum(1), 1.0, rtol=1e-6)
    out.check_guard()
    lse.check_guard()


@pytest.mark.parametrize("c", TABLES["dirichlet"] + TABLES["dirichlet_bound"], ids=case_id)
def test_dirichlet_expectation(ctx, c):
    dev = ctx.device
    rows, cols = c["rows"], c["cols"]
    lam = V.place(dirichlet_data(c), c["lay"], dev)
    out = V.out_like((rows, cols), F32, D0, dev)
    want = reference(c["entry"], c)
    if c["entry"] == "dirichlet":
        ctx.call("bsc_dirichlet_expectation", lam.ptr, rows, cols, lam.strides[0], out.ptr)
        ctx.sync()
    else:
        bound = V.out_like((1,), F64, D0, dev)
        ctx.call("bsc_dirichlet_expectation_bound", lam.ptr, rows, cols, lam.strides[0], 0.01, out.ptr, bound.ptr)
        ctx.sync()
        npt.assert_allclose(bound.numpy()[0], want["bound"], rtol=1e-11, atol=1e-9)
        bound.check_guard()
    npt.assert_allclose(out.numpy(), want["out"], rtol=2e-6, atol=1e-37)
    out.check_guard()


@_params("natgrad_2d")
def test_natgrad_update_f32_2d(ctx, c):
    dev = ctx.device
    eta, msg = natgrad_data(c)
    e = V.place(eta, c["leta"], dev, inout=True)
    m = V.place(msg, c["lmsg"], dev)
    ctx.call("bsc_natgrad_update_f32_2d", e.ptr, e.strides[0], 0.01, m.ptr, m.strides[0], c["rows"], c["cols"], 1.7, 0.3,
             None, 0, None, None, None)
    ctx.sync()
    # three float32 roundings of positive terms: rtol 1e-6 (test_fusion_gpu.test_... X * u + 1: rtol 1e-6, atol 1e-6)
    npt.assert_allclose(e.numpy(), reference("natgrad_2d", c)["eta"], rtol=1e-6, atol=1e-6)
    e.check_guard()


@_params("suffstats")
def test_suffstats_normal(ctx, c):
    dev = ctx.device
    x = V.place(suffstats_data(c), Layout(base_off=c["off"]), dev)
    stats = V.out_like((3,), F64, D0, dev)
    ctx.call("bsc_suffstats_normal", x.ptr, c["n"], stats.ptr)
    ctx.sync()
    npt.assert_allclose(stats.numpy(), reference("suffstats", c)["stats"], rtol=1e-13)
    stats.check_guard()


@pytest.mark.parametrize("c", TABLES["lda"] + TABLES["lda_bound"], ids=case_id)
def test_lda_sstats(ctx, alt, c):
    cx = ctx if c["stream"] else alt(lda_stream=0)
    dev = ctx.device
    entry = "lda_bound" if c["bound"] else "lda"
    C, Th, Bt = lda_data(c)
    want = reference(entry, c)
    cv, th, bt = V.place(C, c["c"], dev), V.place(Th, c["th"], dev), V.place(Bt, c["bt"], dev)
    out = V.out_like((c["K"], c["V"]), F32, c["o"], dev)
    args = (cv.ptr, cv.strides[0], c["docs"], c["V"], c["K"], th.ptr, th.strides[0], bt.ptr, bt.strides[0], out.ptr,
            out.strides[0])
    if c["bound"]:
        ll = V.out_like((1,), F64, D0, dev)
        cx.call("bsc_lda_sstats_bound", *args, ll.ptr)
        cx.sync()
        assert abs(ll.numpy()[0] - want["ll"]) <= 3e-6 * want["ll_scale"] + 1e-9, (ll.numpy()[0], want["ll"])
        ll.check_guard()
    else:
        cx.call("bsc_lda_sstats", *args)
        cx.sync()
    npt.assert_allclose(out.numpy(), want["sstats"], rtol=3e-5, atol=1e-6)
    out.check_guard()


@pytest.mark.parametrize("c", TABLES["lda_csc"] + TABLES["lda_csc_bound"], ids=case_id)
def test_lda_sstats_csc(ctx, alt, c):
    import scipy.sparse as sp
    import torch
    cx = ctx if c["fast"] else alt(csc_fast=0)
    dev = ctx.device
    entry = "lda_csc_bound" if c["bound"] else "lda_csc"
    C, Th, Bt = lda_data(c, 0.05)
    want = reference(entry, c)
    csc = sp.csc_matrix(C)
    colptr = torch.from_numpy(csc.indptr.astype(np.int64)).to(dev)
    rowidx = torch.from_numpy(csc.indices.astype(np.int32)).to(dev)
    vals = torch.from_numpy(csc.data.astype(F32)).to(dev)
    th, bt = V.place(Th, c["th"], dev), V.place(Bt, D0, dev)
    out = V.out_like((c["K"], c["V"]), F32, D0, dev)
    args = (colptr, rowidx, vals, c["docs"], c["V"], c["K"], th.ptr, th.strides[0], bt.ptr, bt.strides[0], out.ptr,
            out.strides[0])
    if c["bound"]:
        ll = V.out_like((1,), F64, D0, dev)
        cx.call("bsc_lda_sstats_csc_bound", *args, ll.ptr)
        cx.sync()
        assert abs(ll.numpy()[0] - want["ll"]) <= 3e-6 * want["ll_scale"] + 1e-9, (ll.numpy()[0], want["ll"])
        ll.check_guard()
    else:
        cx.call("bsc_lda_sstats_csc", *args)
        cx.sync()
    npt.assert_allclose(out.numpy(), want["sstats"], rtol=3e-5, atol=1e-6)
    out.check_guard()


@_params("mog")
def test_mog_estep(ctx, c):
    dev = ctx.device
    X, Wmat, cvec = mog_data(c)
    N, D, K = c["N"], c["D"], c["K"]
    xv = V.place(X, c["lay"], dev)
    stats = V.out_like((K, 1 + 2 * D), F64, D0, dev)
    lse = V.out_like((1,), F64, D0, dev)
    ctx.call("bsc_mog_estep", xv.ptr, xv.strides[0], N, D, K, ctx.to_device(Wmat), ctx.to_device(cvec), stats.ptr, lse.ptr)
    ctx.sync()
    want = reference("mog", c)
    X64 = np.abs(X.astype(F64))
    scale = np.concatenate([[max(N, 1)], X64.sum(0) + 1e-9, (X64 ** 2).sum(0) + 1e-9])
    assert (np.abs(stats.numpy() - want["stats"]) <= 3e-5 * scale[None, :] + 1e-9).all()
    npt.assert_allclose(lse.numpy()[0], want["lse"], rtol=3e-6, atol=1e-4)
    stats.check_guard()
    lse.check_guard()


def _y_operand(c, yv, dev):
    """-> (view, (row stride, column stride)) of the second operand over the [R, C] index space."""
    R, C = c["shape"]
    y = c["y"]
    if y == "rowvec":
        v = V.place(yv, D0, dev)
        return v, (0, 1)
    if y == "percol":
        v = V.place(yv, D0, dev)
        return v, (1, 0)
    if y == "scalar":
        v = V.place(yv, D0, dev)
        return v, (0, 0)
    if y == "diag":
        v = V.place(yv, D0, dev)
        return v, (v.strides[0] + 1, 0)
    lay = {"dense": D0, "transposed": Layout(transpose=True), "offset": Layout(base_off=1), "oddld": Layout(ld_extra=1)}[y]
    v = V.place(yv, lay, dev)
    return v, v.strides


@_params("map")
def test_map_family(ctx, alt, c):
    cx = ctx if c["flat"] else alt(fused_map_flat=0)
    dev = ctx.device
    R, C = c["shape"]
    x, yv = map_data(c)
    want = reference("map", c)["out"]
    xv = V.place(x, c["x"], dev)
    op = c["op"]
    COPY, ADD = 6, 0
    if op in ("map", "elemwise", "convert"):
        out = V.out_like((R, C), F32, c["out"], dev)
    else:
        n_out = C if op == "colsum" else R
        out = V.out_like((n_out,), F32, c["out"] if op != "sum" else D0, dev)
    if op == "convert":
        cx.call("bsc_convert", 0, 0, 2, _i64((R, C)), xv.ptr, _i64(xv.strides), out.ptr, _i64(out.strides))
    elif op == "sum":
        cx.call("bsc_sum", 0, 1, _i64((R,)), _i64((xv.strides[0],)), 1, _i64((C,)), _i64((xv.strides[1],)), xv.ptr, out.ptr)
    else:
        y, ys = _y_operand(c, yv, dev)
        ptrs = (ctypes.c_void_p * 2)(xv.ptr, y.ptr)
        if op == "elemwise":
            cx.call("bsc_elemwise", ADD, 0, 2, _i64((R, C)), out.ptr, _i64(out.strides), 2, ptrs,
                    _i64(tuple(xv.strides) + tuple(ys)))
        else:
            pre_ops = (ctypes.c_int32 * 2)(COPY, COPY)
            pre_args = (ctypes.c_double * 2)(0.0, 0.0)
            if op == "map":
                keep, red, ks, rs_ = (R, C), (), tuple(xv.strides) + tuple(ys), ()
            elif op == "rowsum":
                keep, red, ks, rs_ = (R,), (C,), (xv.strides[0], ys[0]), (xv.strides[1], ys[1])
            else:
                keep, red, ks, rs_ = (C,), (R,), (xv.strides[1], ys[1]), (xv.strides[0], ys[0])
            cx.call("bsc_map_reduce", 0, ADD, len(keep), _i64(keep), len(red), _i64(red), 2, ptrs, _i64(ks), _i64(rs_),
                    pre_ops, pre_args, 0.5, 0.25, COPY, 0.0, out.ptr, _i64(out.strides))
    cx.sync()
    if op in ("map", "elemwise", "convert"):
        npt.assert_allclose(out.numpy(), want, rtol=1e-6, atol=1e-6)
    else:
        npt.assert_allclose(out.numpy(), want, rtol=1e-5)              # every term positive: 1e-5 * sum|terms|
    out.check_guard()


# =====================================================================================================
# entry points that must REFUSE a misaligned base or a leading dimension that is not a multiple of 4:
# BayesicHipError with the library's message, outputs untouched bit for bit, the next valid call right
# =====================================================================================================
BAD_LAYOUTS = [Layout(base_off=1), Layout(base_off=2), Layout(base_off=3), Layout(ld_extra=1), Layout(ld_extra=2),
               Layout(ld_extra=3)]
BAD_BASES = BAD_LAYOUTS[:3]                                   # for operands that have no leading dimension to pass


def _bad(which_and_layouts):
    return [pytest.param(w, l, id="%s-%s" % (w, l.describe())) for w, ls in which_and_layouts for l in ls]


def _untouched(view):
    bits = view.buf.view(V._SIGNED[view.np_dtype]).cpu().numpy().view(V._BITS[view.np_dtype])
    return bool((bits == V.SENTINEL[view.np_dtype]).all())


def _int32_at(values, base_off, dev):
    """An int32 device vector whose first element lies base_off elements past a 16-byte boundary."""
    import torch
    buf = torch.zeros(V.GUARD + base_off + len(values), dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[V.GUARD + base_off:]
    t.copy_(torch.from_numpy(values))
    return t


@pytest.mark.parametrize("sweep", [False, True], ids=["pass", "sweep"])
@pytest.mark.parametrize("which,lay", _bad([("X", BAD_LAYOUTS), ("W", BAD_BASES)]))
def test_blr_data_pass_refuses(ctx, which, lay, sweep):
    from bayesic_amd._ffi import BayesicHipError
    dev = ctx.device
    rs = np.random.RandomState(5)
    B, D, S = 4097, 256 if sweep else 64, 3
    X = rs.standard_normal((B, D)).astype(F32)
    y = rs.standard_normal(B).astype(F32)
    W = (rs.standard_normal((S, D)) / 8).astype(F32)
    name = "bsc_blr_data_pass_sweep" if sweep else "bsc_blr_data_pass"
    tail = (1,) if sweep else ()
    msg = "X and W must be 16-byte aligned" if lay.base_off else r"ldx=\d+ must be >= D, % 4 == 0"
    for bad in (True, False):
        xv = V.place(X, lay if bad and which == "X" else D0, dev)
        wv = V.place(W, lay if bad and which == "W" else D0, dev)
        Q, G = V.out_like((S,), F64, D0, dev), V.out_like((S, D), F64, D0, dev)
        args = (xv.ptr, xv.strides[0], ctx.to_device(y), B, D, wv.ptr, S, Q.ptr, G.ptr) + tail
        if bad:
            with pytest.raises(BayesicHipError, match=msg):
                ctx.call(name, *args)
            ctx.sync()
            assert _untouched(Q) and _untouched(G)
        else:
            ctx.call(name, *args)
            ctx.sync()
            q_ref, g_ref = svi.blr_data_pass(X, y, W)
            X64 = X.astype(F64)
            size = np.abs(y.astype(F64))[:, None] + np.abs(X64) @ np.abs(W.astype(F64)).T
            assert (np.abs(Q.numpy() - q_ref) <= 3e-6 * (q_ref + 1e-1 * (size ** 2).sum(0))).all()
            scale = np.sqrt(q_ref)[:, None] * np.sqrt((X64 ** 2).sum(0))[None, :] + 1e-12
            g_size = (size[:, :, None] * np.abs(X64)[:, None, :]).sum(0)
            assert (np.abs(G.numpy() - g_ref) <= 2e-5 * scale + 3e-7 * g_size).all()
            Q.check_guard()
            G.check_guard()


@pytest.mark.parametrize("which,lay", _bad([("X", BAD_LAYOUTS), ("y", BAD_BASES), ("g", BAD_BASES), ("Wz", BAD_BASES)]))
def test_logreg_bbvi_loglik_refuses(ctx, which, lay):
    from bayesic_amd._ffi import BayesicHipError
    dev = ctx.device
    rs = np.random.RandomState(6)
    N, D, G = 1000, 64, 7
    X = rs.standard_normal((N, D)).astype(F32)
    y = (rs.uniform(size=N) < 0.4).astype(F32)
    g = rs.randint(G, size=N).astype(np.int32)
    Wz = (rs.standard_normal((64, D)) / 8).astype(F32)
    Bz = rs.standard_normal((G, 64)).astype(F32)
    msg = "X, y, g and Wz must be 16-byte aligned" if lay.base_off else r"bad ldx=\d+"
    for bad in (True, False):
        pick = lambda n: lay if bad and which == n else D0
        xv, yv, wv = V.place(X, pick("X"), dev), V.place(y, pick("y"), dev), V.place(Wz, pick("Wz"), dev)
        gv = _int32_at(g, pick("g").base_off, dev)
        ell = V.out_like((64,), F64, D0, dev)
        args = (xv.ptr, xv.strides[0], yv.ptr, gv, N, D, G, wv.ptr, ctx.to_device(Bz), 64, ell.ptr)
        if bad:
            with pytest.raises(BayesicHipError, match=msg):
                ctx.call("bsc_logreg_bbvi_loglik", *args)
            ctx.sync()
            assert _untouched(ell)
        else:
            ctx.call("bsc_logreg_bbvi_loglik", *args)
            ctx.sync()
            npt.assert_allclose(ell.numpy(), svi.logreg_loglik(X, y, g, Wz, Bz), rtol=5e-6, atol=1e-4)
            ell.check_guard()


@pytest.mark.parametrize("stats", [False, True], ids=["rows", "stats"])
@pytest.mark.parametrize("which,lay", _bad([("A", BAD_LAYOUTS), ("R", BAD_LAYOUTS)]))
def test_gemm_softmax_refuses(ctx, which, lay, stats):
    """A (input) and R (the output written with 16-byte stores): a base off a 16-byte boundary, lda / ldr % 4 != 0."""
    from bayesic_amd._ffi import BayesicHipError
    dev = ctx.device
    rs = np.random.RandomState(7)
    rows, K, N = 257, 24, 12
    A = rs.standard_normal((rows, K)).astype(F32)
    B = (rs.standard_normal((K, N)) * 1.5).astype(F32)
    name = "bsc_gemm_softmax_stats" if stats else "bsc_gemm_softmax_rows"
    if which == "A":
        msg = name + (": A.* 16-byte aligned" if lay.base_off else r": lda=\d+")
    elif stats:
        msg = name + ": R must be 16-byte aligned with ldr % 4 == 0"
    else:
        msg = name + (": A and R must be 16-byte aligned" if lay.base_off else r": lda=\d+ ldr=\d+")
    logits = A.astype(F64) @ B.astype(F64)
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    want = e / e.sum(1, keepdims=True)
    for bad in (True, False):
        av = V.place(A, lay if bad and which == "A" else D0, dev)
        R = V.out_like((rows, N), F32, lay if bad and which == "R" else D0, dev)
        if stats:
            # ldst carries no alignment condition (bsc_rowsoftmax.hip: ldst >= K only): K + 1 is accepted and right
            st, tot = V.out_like((N, K), F32, Layout(ld_extra=1), dev), V.out_like((1,), F64, D0, dev)
            args = (av.ptr, av.strides[0], rows, K, ctx.to_device(B), N, 1, N, 1.0, None, R.ptr, R.strides[0], st.ptr,
                    st.strides[0], tot.ptr)
            outs = (R, st, tot)
        else:
            lse, cross = V.out_like((rows,), F32, D0, dev), V.out_like((rows,), F32, D0, dev)
            args = (av.ptr, av.strides[0], rows, K, ctx.to_device(B), N, 1, N, 1.0, R.ptr, R.strides[0], lse.ptr, cross.ptr)
            outs = (R, lse, cross)
        if bad:
            with pytest.raises(BayesicHipError, match=msg):
                ctx.call(name, *args)
            ctx.sync()
            assert all(_untouched(o) for o in outs)
        else:
            ctx.call(name, *args)
            ctx.sync()
            npt.assert_allclose(R.numpy(), want, rtol=2e-5, atol=2e-6)          # test_softmax_gpu's tolerance
            if stats:           # test_softmax_stats_gpu's bound: 3e-6 of sum_r |R| |A|
                s_ref, s_bound = want.T @ A.astype(F64), want.T @ np.abs(A.astype(F64))
                assert (np.abs(st.numpy() - s_ref) <= 3e-6 * s_bound + 1e-6).all()
            for o in outs:
                o.check_guard()


@pytest.mark.parametrize("which", ["R", "X", "Y"])
@pytest.mark.parametrize("lay", BAD_LAYOUTS, ids=Layout.describe)
def test_weighted_outer_refuses(ctx, lay, which):
    from bayesic_amd._ffi import BayesicHipError
    dev = ctx.device
    rs = np.random.RandomState(8)
    N, K, D, E = 1000, 8, 12, 4
    R = rs.standard_normal((N, K)).astype(F32)
    X = rs.standard_normal((N, D)).astype(F32)
    Y = rs.standard_normal((N, E)).astype(F32)
    R64, X64, Y64 = (a.astype(F64) for a in (R, X, Y))
    want = np.einsum("nk,nd,ne->kde", R64, X64, Y64)
    bound = np.einsum("nk,nd,ne->kde", np.abs(R64), np.abs(X64), np.abs(Y64))
    for bad in (True, False):
        lays = {n: (lay if bad and n == which else D0) for n in "RXY"}
        r, x, y = V.place(R, lays["R"], dev), V.place(X, lays["X"], dev), V.place(Y, lays["Y"], dev)
        out = V.out_like((K, D, E), F32, D0, dev)
        args = (r.ptr, r.strides[0], x.ptr, x.strides[0], y.ptr, y.strides[0], N, K, D, E, 1.0, out.ptr)
        if bad:
            with pytest.raises(BayesicHipError, match="bsc_weighted_outer: operands must be 16-byte aligned"):
                ctx.call("bsc_weighted_outer", *args)
            ctx.sync()
            assert _untouched(out)
        else:
            ctx.call("bsc_weighted_outer", *args)
            ctx.sync()
            assert (np.abs(_f64(out.t) - want) <= 2e-5 * bound + 1e-30).all()
            out.check_guard()


# =====================================================================================================
# gates on SPAN: operands whose rows lie millions of floats apart (device-allocated, only the rows in use
# filled, values only -- no guard on buffers of this size)
# =====================================================================================================
K_LIMIT = ((1 << 29) - 32) // 127          # dma_ok, k-contiguous operand: (127 s_mn + 32) * 4 < 2^31
M_LIMIT = ((1 << 29) - 128) // 31          # dma_ok, m-contiguous operand: (31 s_k + 128) * 4 < 2^31
TN_K = 20000
TN_LIMIT = ((1 << 29) - TN_K) // 15        # skinny TN: sa_m * 15 + K < 2^29 (binds before ld < 2^26)


SPAN_CASES = [
    # id, (M, N, K), which operand is spread, its big stride
    ("gemm-kcontig-below", (128, 384, 160), "A_rows", K_LIMIT // 4 * 4 - 4),
    ("gemm-kcontig-above", (128, 384, 160), "A_rows", K_LIMIT // 4 * 4 + 4),
    ("gemm-mcontig-below", (128, 384, 32), "A_cols", M_LIMIT // 4 * 4 - 4),
    ("gemm-mcontig-above", (128, 384, 32), "A_cols", M_LIMIT // 4 * 4 + 4),
    ("skinny-tn-below", (4, 64, TN_K), "A_rows", TN_LIMIT // 4 * 4 - 4),
    ("skinny-tn-above", (4, 64, TN_K), "A_rows", TN_LIMIT // 4 * 4 + 4),
]


def test_span_cases_straddle_the_limits():
    """(Needs no device, but lives with the cases.)  Below: the gate's own inequality holds; above: it does not."""
    for name, (M, N, K), how, stride in SPAN_CASES:
        if name.startswith("gemm-kcontig"):
            holds = (127 * stride + 32) * 4 < (1 << 31)
        elif name.startswith("gemm-mcontig"):
            holds = (31 * stride + 128) * 4 < (1 << 31)
        else:
            holds = stride * 15 + K < (1 << 29) and stride < (1 << 26)
        assert holds == name.endswith("below") and stride % 4 == 0, name
        rows = M if how == "A_rows" else K
        assert rows * stride * 4 < 8 * (1 << 30)


@pytest.mark.parametrize("name,shape,how,stride", SPAN_CASES, ids=[c[0] for c in SPAN_CASES])
def test_span_gates(ctx, name, shape, how, stride):
    import torch
    dev = ctx.device
    M, N, K = shape
    rs = np.random.RandomState(len(name) + stride % 1000)
    A = rs.standard_normal((M, K)).astype(F32)
    B = rs.standard_normal((K, N)).astype(F32)
    n_rows, width = (M, K) if how == "A_rows" else (K, M)
    buf = torch.empty((n_rows - 1) * stride + width, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    try:
        stored = torch.as_strided(buf, (n_rows, width), (stride, 1))
        stored.copy_(torch.from_numpy(A if how == "A_rows" else np.ascontiguousarray(A.T)).to(dev))
        sa_m, sa_k = (stride, 1) if how == "A_rows" else (1, stride)
        b = V.place(B, D0, dev)
        out = V.out_like((M, N), F32, D0, dev)
        ctx.call("bsc_gemm_strided_batched", 0, 1, M, N, K, buf.data_ptr(), 0, sa_m, sa_k, b.ptr, 0, *b.strides,
                 out.ptr, 0, *out.strides)
        ctx.sync()
        got = _f64(out.t)
    finally:
        del buf, stored
        torch.cuda.empty_cache()
    A64, B64 = A.astype(F64), B.astype(F64)
    err = np.abs(got - A64 @ B64)
    bound = np.abs(A64) @ np.abs(B64)
    print("max err / bound", float((err / bound).max()))
    assert (err <= 1e-5 * bound + 1e-30).all()


# =====================================================================================================
# one level up: the executor and the engines on the same views.  The fused entry points are refused (the
# executor checks their envelope and does not call them); the general route must answer and be RIGHT.
# =====================================================================================================
@pytest.mark.parametrize("lay", [D0] + BAD_LAYOUTS, ids=Layout.describe)
def test_three_factor_contraction_on_views_takes_the_general_route(ctx, lay):
    """sum_n R_nk X_nd X_ne with R and X device views: bsc_weighted_outer on aligned operands, the general
    contraction otherwise -- either way equal to the host float64 evaluation of the same expression within the
    weighted outer product's own bound (2e-5 of sum |R| |X| |X|)."""
    from bayesic_amd.algebra import dimshuffle, sum as asum, var
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from oracle.einsum_eval import NumpyBackend
    from test_fusion_gpu import Counting
    rs = np.random.RandomState(9)
    N, K, D = 5000, 8, 12
    R_ = rs.dirichlet(np.ones(K), N).astype(F32)
    X_ = rs.standard_normal((N, D)).astype(F32)
    R, X = var("R", ndim=2), var("X", ndim=2)
    second = asum(dimshuffle(R, 0, 1, "x", "x") * dimshuffle(X, 0, "x", 1, "x") * dimshuffle(X, 0, "x", "x", 1), axis=0)
    want = second.compile(NumpyBackend(F64))(R=R_.astype(F64), X=X_.astype(F64))
    bound = np.einsum("nk,nd,ne->kde", np.abs(R_.astype(F64)), np.abs(X_.astype(F64)), np.abs(X_.astype(F64)))
    for r_lay, x_lay in ((lay, D0), (D0, lay)):
        rv, xv = V.place(R_, r_lay, ctx.device), V.place(X_, x_lay, ctx.device)
        f = second.compile(DeviceBackend(ctx))
        with Counting(ctx) as c:
            got = f(R=rv.t, X=xv.t)
        assert c.count("bsc_weighted_outer") == (1 if lay.dense else 0), c.calls
        assert got.shape == (K, D, D)
        assert (np.abs(got - want) <= 2e-5 * bound + 1e-30).all()


@pytest.mark.parametrize("lay", [D0] + BAD_LAYOUTS, ids=Layout.describe)
def test_softmax_of_a_product_on_a_view_takes_the_general_route(ctx, lay):
    """A Categorical node's update softmax_rows(X . Y) with X a device view: ONE bsc_gemm_softmax_rows launch on an
    aligned X, the product and bsc_softmax_rows otherwise; responsibilities against float64 numpy at the fused
    kernel's own tolerance (tests/test_softmax_gpu.py: rtol 2e-5, atol 2e-6)."""
    from bayesic_amd.algebra import dot, var
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from test_fusion_gpu import Counting
    rs = np.random.RandomState(10)
    rows, K, N = 4099, 24, 12
    X_ = rs.standard_normal((rows, K)).astype(F32)
    Y_ = (rs.standard_normal((K, N)) * 1.5).astype(F32)
    logits = X_.astype(F64) @ Y_.astype(F64)
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    want = e / e.sum(1, keepdims=True)
    be = DeviceBackend(ctx)
    xv = V.place(X_, lay, ctx.device)
    with Counting(ctx) as c:
        R, lse, cross, _ = be.evaluate_softmax_rows(dot(var("X", ndim=2), var("Y", ndim=2)),
                                                    dict(X=xv.t, Y=ctx.to_device(Y_)))
    ctx.sync()
    if lay.dense:
        assert c.count("bsc_gemm_softmax_rows") == 1 and c.count("bsc_softmax_rows") == 0, c.calls
    else:
        assert c.count("bsc_gemm_softmax_rows") == 0 and c.count("bsc_softmax_rows") == 1 and \
            c.count("bsc_gemm_strided_batched") + c.count("bsc_gemm_epilogue") == 1, c.calls
    npt.assert_allclose(R.cpu().numpy(), want, rtol=2e-5, atol=2e-6)
    npt.assert_allclose(lse.cpu().numpy(), (m + np.log(e.sum(1, keepdims=True)))[:, 0], rtol=0,
                        atol=1e-5 * (np.abs(logits).max() + 1.0))


@pytest.mark.parametrize("lay", [D0, Layout(base_off=1), Layout(ld_extra=1), Layout(base_off=3, ld_extra=3)],
                         ids=Layout.describe)
def test_mixture_local_step_on_a_view_is_right(ctx, lay):
    """The derived mean-field engine of the diagonal mixture with its data a device VIEW.  The executor copies the
    view's columns into the wide operand [X | X^2 | 1] it owns (aligned, ld % 4 == 0), so bsc_gemm_softmax_stats
    runs on that copy for every layout of X and is never handed the view; what must hold is that the copy reads
    the view right.  Against the float64 oracle step at tests/test_softmax_stats_gpu.py's bound (1e-3 of
    max(|eta|, 1))."""
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference.mixture import DiagonalMixtureVMP
    from test_fusion_gpu import Counting
    n, d, k = 20000, 16, 8
    X, _, _ = svi.make_cfg3(n, d, k)
    eta0 = svi.mog_prior_eta(k, d)
    eta = svi.mog_init_eta(X[:500], k, d, seed=2)
    init = svi.mog_unpack(eta, k, d)
    xv = V.place(X.astype(F32), lay, ctx.device)
    model = DiagonalMixtureVMP(xv.t, k, n_total=10.0 * n, init=init, backend=DeviceBackend(ctx), route="derived")
    for t in range(1, 3):
        rho = (t + 1.0) ** -0.6
        with Counting(ctx) as c:
            model.step(rho)
        eta, _, _ = svi.mog_svi_step(eta, eta0, X, 10.0 * n, rho, k, d)
    assert c.count("bsc_gemm_softmax_stats") == 1 and c.count("bsc_gemm_softmax_rows") == 0, c.calls
    got = model.eta_fused_layout()
    scale = np.maximum(np.abs(eta), 1.0)
    assert (np.abs(got - eta) <= 1e-3 * scale).all(), np.abs((got - eta) / scale).max()
