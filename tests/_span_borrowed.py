"""Entry points of tests/test_span_routes_gpu.py whose dense tests already own a runner that uploads host arrays and an
assertion with the entry point's tolerance: the grouped, weighted and learned-scalar regression passes and their
predictive passes.  Their runners are used AS THEY ARE through `Borrow`, a stand-in for the context that hands the runner
the matrix where it already lies (spread in the wide buffer, or compact) instead of uploading it, and puts that
matrix's leading dimension into the call; outputs the runner asks for with ctx.zeros come NaN-prefilled and are kept
for the refusal checks.  Each entry is (make, run, check) as in the test file:

  make(c) -> dict with "M" (the [rows, width] matrix that is spread) and "args" (the dense test's inputs, M among them)
  run(cx, ptr, ld, c, d) -> name -> numpy
  check(c, d, got) -> printed figures (the borrowed assertions print their own)

Tolerances, by the assertion that is called:
  bsc_glm_data_pass_obs                test_glm_obs_gpu._assert_close
  bsc_glm_data_pass_groups             test_glm_group_gpu._assert_close
  bsc_glm_nb_data_pass                 test_glm_nb_gpu._assert_close
  bsc_glm_weibull_data_pass_interval   test_glm_weibull_interval_gpu._check's (_glm_weibull_interval_ref.bounds, EPS)
  bsc_glm_ordinal_data_pass            test_glm_ordinal_gpu._assert_close
  bsc_predict_pass_offset              test_glm_obs_gpu._assert_predict
  bsc_predict_pass_groups              test_predict_group_gpu._assert_inside
  bsc_lda_sstats                       test_lda_gpu (rtol 3e-5, atol 1e-6), on test_view_routes_gpu.lda_data
"""
import importlib

import numpy as np

F32 = np.float32


class _Ref(object):
    """What the borrowed runner holds in place of the uploaded matrix."""

    def __init__(self, ptr, ld, shape):
        self.ptr, self.ld, self.shape = ptr, ld, shape

    def stride(self, k):
        return self.ld if k == 0 else 1

    def data_ptr(self):
        return self.ptr


class Borrow(object):
    def __init__(self, cx, M, ptr, ld, outputs):
        self._cx, self._M, self._ref, self._outputs = cx, M, _Ref(ptr, ld, M.shape), outputs

    def __getattr__(self, name):
        return getattr(self._cx, name)

    def to_device(self, array, dtype=None):
        a = array
        if isinstance(a, np.ndarray) and a.dtype == self._M.dtype and a.shape == self._M.shape and \
                (a is self._M or np.array_equal(a, self._M)):
            return self._ref
        return self._cx.to_device(array, dtype)

    def zeros(self, shape, dtype=None):
        import torch
        t = torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype or torch.float32,
                       device=self._cx.device)
        self._outputs.append(t)
        return t

    def call(self, name, *args):
        args = list(args)
        at = [i for i, a in enumerate(args) if a is self._ref]
        assert len(at) <= 1, "the spread matrix is one argument of %s" % name
        if at:                                                                  # (not in the calls that only plan)
            args[at[0]], args[at[0] + 1] = self._ref.ptr, self._ref.ld        # (pointer, leading dimension)
        self._cx.call(name, *args)


def _named(got, names):
    return got if isinstance(got, dict) else dict(zip(names, got))


def borrowed(module, make, run, check, names):
    """(make, run, check) around a dense test module's own runner and assertion; `outputs`: the test file's list."""
    def load():
        return importlib.import_module(module)

    def make_(c):
        args = make(load(), c)
        return dict(M=args[0], args=args)

    def run_(cx, ptr, ld, c, d, outputs):
        return _named(run(load(), Borrow(cx, d["M"], ptr, ld, outputs), c, d["args"]), names)

    def check_(c, d, got):
        check(load(), c, d["args"], tuple(got[k] for k in names))
        return ["(figures printed by %s)" % module]

    return make_, run_, check_


def _seed(c):
    return 7 * c["rows"] + c["D"] + c["S"]


GLM_OBS = borrowed(
    "test_glm_obs_gpu", lambda m, c: m._inputs(c["link"], c["rows"], c["D"], c["S"], _seed(c), "both"),
    lambda m, cx, c, a: m._pass(cx, c["link"], *a), lambda m, c, a, got: m._assert_close(c["link"], got, *a), ("ell", "G"))


def _groups_run(m, cx, c, a):
    """test_glm_group_gpu._pass, written out: its outputs are not made with ctx.zeros, so they are made here."""
    import torch
    X, y, g, W, Bm, o, v = a
    (B, D), S, J = X.shape, W.shape[0], c["J"]
    gd = m._dev_vec(cx, g, dtype=np.int32, sentinel=-1)
    plan, _ = m._plan(cx, gd, B, J)
    ell, G, H = cx.zeros(S, torch.float64), cx.zeros((S, D), torch.float64), cx.zeros((S, J), torch.float64)
    cx.call("bsc_glm_data_pass_groups", m.CODE[c["link"]], cx.to_device(X), D, m._dev_vec(cx, y), m._dev_vec(cx, o),
            m._dev_vec(cx, v), gd, plan, B, D, J, cx.to_device(W), cx.to_device(m.ref.chunked(Bm)), S, ell, G, H)
    cx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), H.cpu().numpy()


GLM_GROUPS = borrowed(
    "test_glm_group_gpu", lambda m, c: m._inputs(c["link"], c["rows"], c["D"], c["J"], c["S"], _seed(c)), _groups_run,
    lambda m, c, a, got: m._assert_close(c["link"], got, a[0], a[1], a[2], c["J"], *a[3:]), ("ell", "G", "H"))


GLM_NB = borrowed(
    "test_glm_nb_gpu", lambda m, c: m.ref.make_inputs(c["rows"], c["D"], c["S"], _seed(c), "both"),
    lambda m, cx, c, a: m._pass(cx, *a), lambda m, c, a, got: m._assert_close(got, *a), ("ell", "G", "T"))


def _weibull_check(m, c, a, got):
    want, bnd = m.ref.data_pass(*a), m.ref.bounds(*a)
    ratios = []
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (m.ref.EPS * b + 1e-300)).max()))
    print("%s: error / tolerance ell %.3g, G %.3g, T %.3g" % (c["id"], *ratios))
    for r, name in zip(ratios, ("ell", "G", "T")):
        assert r <= 1.0, (name, r)


WEIBULL_INTERVAL = borrowed(
    "test_glm_weibull_interval_gpu", lambda m, c: m.ref.make_inputs(c["rows"], c["D"], c["S"], _seed(c), "both", "mixed"),
    lambda m, cx, c, a: m._pass(cx, *a), _weibull_check, ("ell", "G", "T"))


# ---- written out: the ordinal pass (either of its two matrices spread) and the two predictive passes -----------------
def _nan(cx, shape, dtype, outputs):
    import torch
    t = torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device=cx.device)
    outputs.append(t)
    return t


def ordinal_make(c):
    import _glm_ordinal_ref as ref
    X, y, Z, o, v = ref.make_inputs(c["rows"] if c["spread"] == "X" else c["B"], c["D"], c["S"], c["K"], seed=_seed(c), mode="both")
    return dict(M=X if c["spread"] == "X" else np.ascontiguousarray(Z), args=(X, y, Z, o, v))


def ordinal_run(cx, ptr, ld, c, d, outputs):
    import torch
    import test_glm_ordinal_gpu as m
    X, y, Z, o, v = d["args"]
    (B, D), S, K = X.shape, Z.shape[0], c["K"]
    P = D + K - 1
    if c["spread"] == "X":
        zd = cx.to_device(np.ascontiguousarray(Z))
        x_args, z_args = (ptr, ld), (zd, P)
    else:
        xd = cx.to_device(X)
        x_args, z_args = (xd, D), (ptr, ld)
    ell, G = _nan(cx, S, torch.float64, outputs), _nan(cx, (S, P), torch.float64, outputs)
    cx.call("bsc_glm_ordinal_data_pass", *x_args, m._dev_labels(cx, y), m._dev_vec(cx, o), m._dev_vec(cx, v), B, D, K, *z_args,
            S, ell, G)
    cx.sync()
    return dict(ell=ell.cpu().numpy(), G=G.cpu().numpy())


def ordinal_check(c, d, got):
    import test_glm_ordinal_gpu as m
    X, y, Z, o, v = d["args"]
    m._assert_close((got["ell"], got["G"]), X, y, Z, c["K"], o, v, what=c["id"])
    return ["(figures printed by test_glm_ordinal_gpu)"]


PREDICT_NAMES = ("mean", "var", "lpd", "lpd_sum")


def _predict_outputs(cx, B, outputs):
    import torch
    out = {k: _nan(cx, B, torch.float32, outputs) for k in PREDICT_NAMES[:3]}
    out["lpd_sum"] = _nan(cx, 1, torch.float64, outputs)
    return out


def predict_offset_make(c):
    import test_glm_obs_gpu as m
    X, y, W, o, _ = m._inputs(c["family"], c["rows"], c["D"], c["S"], _seed(c), "offset")
    return dict(M=X, args=(X, y, W, o))


def predict_offset_run(cx, ptr, ld, c, d, outputs):
    import _predict_ref as pred
    X, y, W, o = d["args"]
    B, D = X.shape
    out = _predict_outputs(cx, B, outputs)
    cx.call("bsc_predict_pass_offset", pred.CODE[c["family"]], ptr, ld, cx.to_device(y), cx.to_device(o), B, D, cx.to_device(W),
            None, W.shape[0], *[out[k] for k in PREDICT_NAMES])
    cx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def predict_offset_check(c, d, got):
    import test_glm_obs_gpu as m
    X, y, W, o = d["args"]
    m._assert_predict(got, c["family"], X, y, W, o)
    return ["(figures printed by test_glm_obs_gpu)"]


def predict_groups_make(c):
    import test_predict_group_gpu as m
    args = m._inputs(c["family"], c["rows"], c["D"], c["J"], c["S"], _seed(c))
    return dict(M=args[0], args=args)


def predict_groups_run(cx, ptr, ld, c, d, outputs):
    import _predict_group_ref as ref
    X, y, g, W, Bt, o = d["args"]
    B, D = X.shape
    out = _predict_outputs(cx, B, outputs)
    bt = cx.to_device(Bt)
    cx.call("bsc_predict_pass_groups", ref.CODE[c["family"]], ptr, ld, cx.to_device(y), cx.to_device(o),
            cx.to_device(np.asarray(g, np.int32)), B, D, c["J"], cx.to_device(W), bt, int(bt.stride(0)), W.shape[0],
            *[out[k] for k in PREDICT_NAMES])
    cx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def predict_groups_check(c, d, got):
    import test_predict_group_gpu as m
    X, y, g, W, Bt, o = d["args"]
    worst = m._assert_inside(c["family"], got, X, y, g, W, Bt, o, what=c["id"])
    return ["%s %.3g" % (k, w) for k, w in worst.items()]


# ---- bsc_lda_sstats: one of C [docs, V], Theta [docs, K], Beta [K, V] spread, the other two and the output compact ---
LDA_DOCS, LDA_V, LDA_K, LDA_VT = 70, 1028, 128, 128       # VT: csrc/bsc_lda.hip, vocabulary columns per workgroup


def lda_holds(which, ld):
    """The stream kernel's inequality on that operand's leading dimension (csrc/bsc_lda.hip, lda_sstats_impl)."""
    if which == "C":
        return (31 * ld + LDA_VT) * 4 < 1 << 31
    if which == "Th":
        return (31 * ld + LDA_K) * 4 < 1 << 31
    return (LDA_K * ld + LDA_V) * 4 < 1 << 32


def lda_first_refused(which):
    """The smallest leading dimension at which lda_holds fails."""
    if which == "Bt":
        return -(-((1 << 30) - LDA_V) // LDA_K)
    return -(-((1 << 29) - (LDA_VT if which == "C" else LDA_K)) // 31)


def lda_make(c):
    import test_view_routes_gpu as vr
    C, Th, Bt = vr.lda_data(dict(id=c["id"], docs=LDA_DOCS, V=LDA_V, K=LDA_K))
    return dict(M=dict(C=C, Th=Th, Bt=Bt)[c["spread"]], args=(C, Th, Bt))


def lda_run(cx, ptr, ld, c, d, outputs):
    import torch
    ops = []
    for name, a in zip(("C", "Th", "Bt"), d["args"]):
        ops.append((ptr, ld) if name == c["spread"] else (cx.to_device(a), a.shape[1]))
    out = _nan(cx, (LDA_K, LDA_V), torch.float32, outputs)
    args = (*ops[0], LDA_DOCS, LDA_V, LDA_K, *ops[1], *ops[2], out, LDA_V)
    if not c["bound"]:
        cx.call("bsc_lda_sstats", *args)
        cx.sync()
        return dict(sstats=out.cpu().numpy())
    ll = _nan(cx, 1, torch.float64, outputs)
    cx.call("bsc_lda_sstats_bound", *args, ll)
    cx.sync()
    return dict(sstats=out.cpu().numpy(), ll=ll.cpu().numpy())


def lda_check(c, d, got):
    from oracle import svi
    want = svi.lda_sstats(*d["args"])
    worst = float((np.abs(got["sstats"] - want) / (3e-5 * np.abs(want) + 1e-6)).max())
    assert worst <= 1.0, worst
    figures = ["sstats %.3g" % worst]
    if c["bound"]:                     # the words' term: 3e-6 of sum C |log phinorm| (test_lda_gpu)
        C, Th, Bt = (a.astype(np.float64) for a in d["args"])
        scale = float((C * np.abs(np.log(Th @ Bt))).sum())
        w_ll = abs(got["ll"][0] - svi.lda_local_bound(*d["args"])) / (3e-6 * scale + 1e-9)
        assert w_ll <= 1.0, w_ll
        figures.append("ll %.3g" % w_ll)
    return figures


ENTRY = {
    "lda": (lda_make, lda_run, lda_check),
    "glm_obs": GLM_OBS, "glm_groups": GLM_GROUPS, "glm_nb": GLM_NB, "weibull_interval": WEIBULL_INTERVAL,
    "ordinal": (ordinal_make, ordinal_run, ordinal_check),
    "predict_offset": (predict_offset_make, predict_offset_run, predict_offset_check),
    "predict_groups": (predict_groups_make, predict_groups_run, predict_groups_check),
}
