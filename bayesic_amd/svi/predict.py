"""Posterior predictive and held-out log density of the fitted regression models, on one fused pass.

Host-side driver of csrc/bsc_predict.hip (include/bayesic_hip.h: bsc_predict_pass).  For S draws of the model's
CURRENT q the pass reads X once and returns, per row, the predictive mean, the predictive variance (law of total
variance over the draws) and, given y, the log predictive density lpd_n = log 1/S sum_s p(y_n | w_s), whose
float64 sum is the held-out score.

Draws (``posterior_draws``): standard normals from bsc_philox_normal on Philox stream 2, step 0, counter and key
as oracle/philox.py lays them out (its streams 0 and 1 belong to the training entry points: 0 = the weights and
every draw of bsc_blr_noise, 1 = the scale latent of bsc_blr_sample), so predicting never repeats training noise.
The transform is parameter-sized and runs once per call: ``_reparam_base.first_draw``, the drivers' own first draw
(float64 on the host), rounded to float32.
    GLMReparamSVI(covariance="diag")  eps [S, D]:      w = m + e^rho eps
    GLMReparamSVI(covariance="full")  eps [S, D]:      w = mu + L eps
    BLRReparamSVI(covariance="diag")  eps [S, D + 1]:  w = m + e^rho eps[:, :D],  xi = a + e^b eps[:, D]
                                      (lam = [m | rho | a | b] re-ordered to the mean-field layout over z = [w | xi])
    BLRReparamSVI(covariance="full")  eps [S, D + 1]:  z = mu + L eps over z = [w | xi]
    SoftmaxReparamSVI                 eps [S, K D]:    the two GLM transforms at width K D, W returned [S, K, D]
                                      (predict() below hands over to its predict(): bsc_softmax_predict_pass)
    NegBinReparamSVI                  eps [S, D + 1]:  w = m + e^rho eps[:, :D],  tau = m_tau + e^{rho_tau} eps[:, D]
                                      (lam is already [m | rho] over z = [w | tau]; bsc_nb_predict_pass)
xi = log s2 is the log-variance of the Gaussian likelihood (``logvar`` of the pass); tau = log phi is the log-dispersion
of the negative binomial and travels in the same slot of the returned pair.

Offsets and weights (logistic, Poisson and negative-binomial models): ``offset`` (or, Poisson, ``exposure`` = e^offset) is added to the
linear predictor in the pass (bsc_predict_pass_offset), so a Poisson ``mean`` is the expected count at that exposure.
A model fitted with an offset refuses to predict without one.  ``weights`` leave every per-row output alone and make
``lpd_sum`` the weighted sum_n v_n lpd_n (float64, on the device, from the lpd vector).
"""
import numpy as np
import torch

from ._obs import batch_obs, check_link
from ._reparam_base import first_draw, float_batch

# include/bayesic_hip.h: BSC_PREDICT_*
FAMILIES = {"gaussian": 0, "logistic": 1, "poisson": 2}
PREDICT_STREAM = 2     # Philox stream of the predictive draws
MAX_SAMPLES = 64       # draws per bsc_predict_pass call

__all__ = ["posterior_draws", "predict", "heldout_lpd", "family_of", "PREDICT_STREAM", "MAX_SAMPLES"]


def family_of(model):
    """The likelihood family of a driver: its GLM link ("negbin" for NegBinReparamSVI), "softmax" for
    SoftmaxReparamSVI, or "gaussian" for BLRReparamSVI."""
    if getattr(model, "n_classes", None) is not None:
        return "softmax"
    link = getattr(model, "link", None)
    if link is not None:
        return link
    if getattr(model, "family", None) is not None:
        raise NotImplementedError(
            "predict: this BLRReparamSVI was built with family=(c0, c_xi, s_q, k_w, beta); the five coefficients of "
            "the log-joint do not identify the likelihood precision (s_q and k_w mix it with the prior's), so the "
            "predictive distribution is not defined by them")
    return "gaussian"


def _check_samples(n_samples):
    S = int(n_samples)
    if S > MAX_SAMPLES:
        raise ValueError("n_samples=%d: one predictive pass takes at most %d draws" % (S, MAX_SAMPLES))
    if S < 1:
        raise ValueError("n_samples must be at least 1")
    return S


def posterior_draws(model, n_samples=64, seed=None):
    """(W float32 [S, D] on the device, logvar float32 [S] or None) from the model's current q; W is [S, K, D] for
    SoftmaxReparamSVI (its guide is over the K D entries, flattened p = k D + d); for NegBinReparamSVI the second
    entry is logphi float32 [S]."""
    S = _check_samples(n_samples)
    family = family_of(model)
    ctx, D = model.ctx, model.D
    if family == "softmax":
        D = model.n_classes * model.D          # the guide's width; the transforms below are the GLM ones
    seed = model.seed if seed is None else int(seed)
    scalar = family in ("gaussian", "negbin")           # a scalar latent rides behind the weights
    P = D + 1 if scalar else D
    eps_d = torch.zeros((S, P), dtype=torch.float64, device=ctx.device)
    ctx.call("bsc_philox_normal", seed, PREDICT_STREAM, 0, S, P, eps_d)
    eps = eps_d.cpu().numpy()
    lam = model.lam.cpu().numpy()
    kind = getattr(model, "covariance_kind", "diag")
    if family == "gaussian" and kind == "diag":         # [m | rho | a | b] -> [m a | rho b] over z = [w | xi]
        lam = np.concatenate([lam[:D], lam[2 * D:2 * D + 1], lam[D:2 * D], lam[2 * D + 1:]])
    z = first_draw(lam, eps, P, kind)
    W, logvar = (z[:, :D], z[:, D]) if scalar else (z, None)
    if family == "softmax":
        W = W.reshape(S, model.n_classes, model.D)
    Wd = ctx.to_device(np.ascontiguousarray(W, np.float32))
    lvd = None if logvar is None else ctx.to_device(np.ascontiguousarray(logvar, np.float32))
    return Wd, lvd


def _data(model, X, y):
    """The drivers' own checks and messages for a batch (GLMReparamSVI.__init__)."""
    X, y = float_batch(model.ctx, X, y, need_y=False)
    if X.shape[1] != model.D:
        raise ValueError("X has %d columns; the model was fitted at D = %d" % (X.shape[1], model.D))
    if y is not None and y.numel() > 1 and y.stride(0) != 1:
        raise ValueError("y must be contiguous")
    return X, y


def _obs(model, family, B, offset, exposure, weights):
    """The checked offset (log exposure) and weights of a batch of B rows: float32 [B] device tensors or None."""
    if offset is None and exposure is None and getattr(model, "has_offset", False):
        raise ValueError("predict: the model was fitted with an offset (exposure); pass offset= or exposure= for the "
                         "rows to predict -- a silent offset of 0 would return rates per unit exposure that look like "
                         "counts")
    if offset is None and exposure is None and weights is None:
        return None, None
    if family not in ("logistic", "poisson", "negbin"):
        raise ValueError("predict: offset, exposure and weights are for the logistic and Poisson models, not %s" % family)
    check_link("poisson" if family == "negbin" else family, offset, exposure, kept="means")   # a count model's rules
    return batch_obs(model.ctx, B, offset, weights, exposure)


def predict(model, X, y=None, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None):
    """Posterior predictive of ``model`` for the rows of X: a dict of device tensors ``mean`` and ``var`` (float32
    [B]) and, with y, ``lpd`` (float32 [B]) and ``lpd_sum`` (float64 [1]).  ``draws`` = (W, logvar) reuses draws of
    ``posterior_draws``; otherwise n_samples (at most 64) are drawn with ``seed`` (default: the model's).
    ``offset`` / ``exposure`` / ``weights``: float32 [B] (module docstring); with weights ``lpd_sum`` is the weighted
    sum and ``weight_sum`` (float64 [1]) is sum_n v_n."""
    family = family_of(model)
    if family == "softmax":      # its own pass and outputs (prob [B, K] instead of mean and var)
        return model.predict(X, y, n_samples=n_samples, seed=seed, draws=draws)
    offset, weights = _obs(model, family, int(X.shape[0]), offset, exposure, weights)
    if draws is None:
        draws = posterior_draws(model, n_samples, seed)
    W, logvar = draws
    S = _check_samples(W.shape[0])
    X, y = _data(model, X, y)
    ctx = model.ctx
    B = int(X.shape[0])
    ldx = int(X.stride(0)) if B > 1 else max(int(X.stride(0)), model.D)
    dev = ctx.device
    out = {"mean": torch.empty(B, dtype=torch.float32, device=dev),
           "var": torch.empty(B, dtype=torch.float32, device=dev)}
    if y is not None:
        out["lpd"] = torch.empty(B, dtype=torch.float32, device=dev)
        if weights is None:        # (the weighted sum is formed from the lpd vector below)
            out["lpd_sum"] = torch.zeros(1, dtype=torch.float64, device=dev)
    if family == "negbin":       # its own entry point; the offset may be None
        ctx.call("bsc_nb_predict_pass", X, ldx, y, offset, B, model.D, W, logvar, S, out["mean"], out["var"],
                 out.get("lpd"), out.get("lpd_sum"))
    elif offset is None:
        ctx.call("bsc_predict_pass", FAMILIES[family], X, ldx, y, B, model.D, W, logvar, S, out["mean"], out["var"],
                 out.get("lpd"), out.get("lpd_sum"))
    else:
        ctx.call("bsc_predict_pass_offset", FAMILIES[family], X, ldx, y, offset, B, model.D, W, logvar, S,
                 out["mean"], out["var"], out.get("lpd"), out.get("lpd_sum"))
    if weights is not None and y is not None:
        w64 = weights.to(torch.float64)       # a row of weight 0 is dropped by a select, as in the training pass
        out["lpd_sum"] = torch.where(weights > 0, w64 * out["lpd"].to(torch.float64), torch.zeros_like(w64)).sum().reshape(1)
        out["weight_sum"] = w64.sum().reshape(1)
    return out


def heldout_lpd(model, X, y, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None):
    """Mean log predictive density per row of the held-out (X, y): lpd_sum / B, a host float (synchronises).  With
    weights: sum_n v_n lpd_n / sum_n v_n."""
    out = predict(model, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                  weights=weights)
    if "weight_sum" in out:
        return float(out["lpd_sum"].item()) / float(out["weight_sum"].item())
    return float(out["lpd_sum"].item()) / max(int(out["lpd"].shape[0]), 1)
