"""Shared by tests/test_mog_predict_cpu.py and tests/test_mog_predict_gpu.py (numpy / scipy only: no device).

 * The posterior predictive of the mean-field mixture (csrc/bsc_mog_predict.hip, include/bayesic_hip.h) restated in
   float64: the table [m | q | h] and c from eta, the logits from the float32 table and float32 rows ("float32 operands,
   float64 arithmetic": the table's rounding is not charged to the pass), and the per-(row, component) bound quantity
   B_nk = |c_k| + sum_d h_kd log1p(u_nkd) that the tolerances are multiples of.
 * The host's grid rule of bsc_mog_predict_pass and the row counts that reach a wanted number of trips per wave.
 * The simulated data sets and the etas the two suites predict from; computed once, never written to.
"""
import functools

import numpy as np
from scipy.special import gammaln

from oracle import svi

EPS = 2e-5               # of the bound quantity: what the project's device tests use
TIE = 4e-5               # a row is a near-tie when its two largest float64 logits are closer than TIE * max_k B_nk
TIE_CAP = 0.01           # share of a case's rows that may be left out of the label check
PT = 64                  # rows per tile (one per lane) and
WAVES = 4                # waves per workgroup and
WAVES_PER_CU = 16        # resident waves per CU the grid is sized for: PT, P_WAVES, P_WAVES_PER_CU of the kernel
F32_EPS = 2.0 ** -23
F32_TINY = 2.0 ** -126   # the smallest normal float32: v_exp_f32 returns 0 below it


# ---- 0. the mathematics -------------------------------------------------------------------------------------------

def pack(alpha, m, kappa, a, b):
    """Natural parameters in svi/mog.py's layout from (alpha [K], m, kappa, a, b [K, D])."""
    return np.concatenate([alpha - 1.0, (kappa * m).ravel(), kappa.ravel(), (2.0 * a - 1.0).ravel(),
                           (2.0 * b + kappa * m * m).ravel()])


def predictive_table(eta, K, D):
    """-> Pt float64 [K, 3D] = [m | q | h], c float64 [K]."""
    alpha, m, kappa, a, b = svi.mog_unpack(eta, K, D)
    q = kappa / (2.0 * b * (kappa + 1.0))
    h = a + 0.5
    c = np.log(alpha) - np.log(alpha.sum()) + (gammaln(a + 0.5) - gammaln(a) + 0.5 * np.log(q / np.pi)).sum(axis=1)
    return np.concatenate([m, q, h], axis=1), c


def table_f32(eta, K, D):
    Pt, c = predictive_table(eta, K, D)
    return Pt.astype(np.float32), c.astype(np.float32)


def logits(X, Pt, c, chunk=16384):
    """float32 X [N, D], float32 table -> float64 logits [N, K] and bound quantity B [N, K]."""
    X, Pt, c = np.asarray(X), np.asarray(Pt), np.asarray(c)
    assert X.dtype == np.float32 and Pt.dtype == np.float32 and c.dtype == np.float32
    N, D = X.shape
    K = c.shape[0]
    P = Pt.astype(np.float64)
    m, q, h = P[:, :D], P[:, D:2 * D], P[:, 2 * D:]
    c64 = c.astype(np.float64)
    L, B = np.empty((N, K)), np.empty((N, K))
    for i in range(0, N, chunk):
        x = X[i:i + chunk].astype(np.float64)
        t = (h[None] * np.log1p(q[None] * (x[:, None, :] - m[None]) ** 2)).sum(axis=2)
        L[i:i + chunk] = c64[None] - t
        B[i:i + chunk] = np.abs(c64)[None] + t
    return L, B


def predict(X, Pt, c):
    """-> dict(L, B, lpd, R, label, tie): the float64 reference of every output, and the near-tie rows."""
    L, B = logits(X, Pt, c)
    N, K = L.shape
    if N == 0:
        return dict(L=L, B=B, lpd=np.zeros(0), R=L.copy(), label=np.zeros(0, np.int64), tie=np.zeros(0, bool))
    mx = L.max(axis=1, keepdims=True)
    e = np.exp(L - mx)
    s = e.sum(axis=1, keepdims=True)
    top = np.sort(L, axis=1)[:, -2:] if K > 1 else np.concatenate([L - np.inf, L], axis=1)
    tie = (top[:, 1] - top[:, 0]) < TIE * B.max(axis=1)
    return dict(L=L, B=B, lpd=(mx + np.log(s))[:, 0], R=e / s, label=L.argmax(axis=1), tie=tie)


def lpd_bound(ref):
    """|lpd - lpd64| <= EPS sum_k R64_nk B_nk: the first-order image of an EPS * B error on each logit."""
    return EPS * (ref["R"] * ref["B"]).sum(axis=1)


def resp_bound(ref):
    """dR_k = R_k (dl_k - sum_j R_j dl_j) with |dl_j| <= EPS B_j, plus what float32 cannot hold (its rounding, and the
    flush below the smallest normal): |R - R64| <= R64 (EPS (B_k + sum_j R64_j B_j) + 2^-23) + 2^-126."""
    mean_b = (ref["R"] * ref["B"]).sum(axis=1, keepdims=True)
    return ref["R"] * (EPS * (ref["B"] + mean_b) + F32_EPS) + F32_TINY


def student_t_logits(X, eta, K, D):
    """The same logits from scipy.stats.t, component by component (float64 table, float64 rows)."""
    from scipy.stats import t as student
    alpha, m, kappa, a, b = svi.mog_unpack(eta, K, D)
    scale = np.sqrt(b * (kappa + 1.0) / (a * kappa))
    X = np.asarray(X, np.float64)
    L = np.empty((X.shape[0], K))
    for k in range(K):
        L[:, k] = np.log(alpha[k] / alpha.sum()) + student.logpdf(X, df=2.0 * a[k], loc=m[k], scale=scale[k]).sum(axis=1)
    return L


def log1p_f32(u, corrected):
    """float32 chain of one term's log1p(u): the plain log(1 + u), or the corrected quotient log(w) u / (w - 1), w = 1 + u
    (u itself where w == 1), every operation rounded to float32."""
    u = np.asarray(u, np.float32)
    w = (np.float32(1.0) + u).astype(np.float32)
    lw = np.log(w.astype(np.float64)).astype(np.float32)          # (a correctly rounded float32 log: the best case)
    if not corrected:
        return lw
    one = w == np.float32(1.0)
    den = np.where(one, np.float32(1.0), (w - np.float32(1.0)).astype(np.float32))
    ratio = (lw / den).astype(np.float32)
    return np.where(one, u, (u * ratio).astype(np.float32)).astype(np.float32)


# ---- 1. the grid ----------------------------------------------------------------------------------------------------

def grid(N, cu):
    """bsc_mog_predict_pass: 64-row tiles, it = ceil(n_tiles / (16 cu)) trips for every wave, waves = ceil(n_tiles / it)."""
    n_tiles = (N + PT - 1) // PT
    if n_tiles <= 0:
        return dict(n_tiles=0, n_iter=0, waves=0, n_blocks=0)
    max_waves = WAVES_PER_CU * cu
    it = (n_tiles + max_waves - 1) // max_waves
    waves = (n_tiles + it - 1) // it
    return dict(n_tiles=n_tiles, n_iter=it, waves=waves, n_blocks=(waves + WAVES - 1) // WAVES)


def rows_for(n_iter, cu):
    """n_iter - 1 full sweeps of the grid, one full tile and a ragged one of five rows."""
    return (n_iter - 1) * WAVES_PER_CU * cu * PT + PT + 5


# ---- 2. data and etas -------------------------------------------------------------------------------------------------

def _fit(X, K, D, steps, seed):
    """Full-batch unit-step natural gradient (VMP) by the oracle, float64."""
    eta0 = svi.mog_prior_eta(K, D)
    eta = svi.mog_init_eta(X, K, D, seed=seed)
    for _ in range(steps):
        eta, _, _ = svi.mog_svi_step(eta, eta0, X, X.shape[0], 1.0, K, D)
    return eta


@functools.lru_cache(maxsize=None)
def fitted_case(N, D, K):
    """Overlapping clusters (tests/_mixture_ref.estep_overlap_data's kind) and an eta three oracle steps into its fit:
    -> X float32 [N, D], eta."""
    rs = np.random.RandomState(7 * N + 3 * D + K)
    n_fit = max(N, 4 * K, 64)
    centres = rs.standard_normal((K, D)) * 3
    Xf = (centres[rs.randint(K, size=n_fit)] + rs.standard_normal((n_fit, D))).astype(np.float32)
    eta = _fit(Xf, K, D, 3, seed=1)
    X = Xf[:N].copy()
    X.setflags(write=False)
    eta.setflags(write=False)
    return X, eta


PARITY_SHAPES = [(1, 16, 64), (7, 16, 64), (63, 16, 64), (64, 16, 64), (65, 16, 64), (1003, 16, 64), (5000, 16, 33),
                 (4097, 5, 64), (333, 1, 2), (20000, 12, 40), (100, 16, 1), (0, 16, 64)]


@functools.lru_cache(maxsize=None)
def parity_reference(N, D, K):
    X, eta = fitted_case(N, D, K)
    Pt, c = table_f32(eta, K, D)
    return X, eta, Pt, c, predict(X, Pt, c)


@functools.lru_cache(maxsize=None)
def precision_case(N=2000, D=16, K=8):
    """A hand-built eta of a well-fitted mixture at config 3's size: a = 1e5, kappa = 2e5, centres near 170, unit spread
    (b = a) -- h = a + 1/2 multiplies whatever log(1 + u) loses."""
    rs = np.random.RandomState(170)
    m = 170.0 + rs.uniform(-4.0, 4.0, (K, D))
    a = np.full((K, D), 1.0e5)
    eta = pack(np.full(K, 1.0 + N / K), m, np.full((K, D), 2.0e5), a, a.copy())
    X = (m[rs.randint(K, size=N)] + rs.standard_normal((N, D))).astype(np.float32)
    return X, eta


def exact_eta(K, D):
    """Components on the centres of tests/_mixture_ref.estep_exact_data (centres[k, k % D] = 24 (1 + k // D)), unit
    precision, equal weights."""
    k = np.arange(K)
    m = np.zeros((K, D))
    m[k, k % D] = 24.0 * (1 + k // D)
    a = np.full((K, D), 50.0)
    return pack(np.full(K, 10.0), m, np.full((K, D), 1000.0), a, a.copy())


@functools.lru_cache(maxsize=None)
def cluster_data():
    """Five separated clusters in D = 5: 3 000 rows to fit on and 1 000 held out."""
    rs = np.random.RandomState(55)
    centres = rs.standard_normal((5, 5)) * 6.0
    lab = rs.randint(5, size=4000)
    X = (centres[lab] + rs.standard_normal((4000, 5))).astype(np.float32)
    X.setflags(write=False)
    return X[:3000], X[3000:]


@functools.lru_cache(maxsize=None)
def cluster_fit(K):
    """eta of a K-component fit to the 3 000 rows (40 full-batch steps of oracle.svi.mog_svi_step)."""
    eta = _fit(cluster_data()[0], K, 5, 40, seed=2)
    eta.setflags(write=False)
    return eta


def heldout_lpd64(eta, K, X):
    Pt, c = table_f32(eta, K, X.shape[1])
    return float(predict(X, Pt, c)["lpd"].mean())


# float64 margins of the held-out lpd on cluster_data (tests/test_mog_predict_cpu.py recomputes and holds them): the
# device must keep the ordering with half of each
MARGIN_5_OVER_2 = 4.90       # -8.7185 against -13.6218 nats per row
MARGIN_5_OVER_1 = 6.72       # ... against -15.4469
