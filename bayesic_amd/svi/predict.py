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
      ... (covariance="full")         eps [S, D + 1]:  z = mu + L eps over z = [w | tau], so that tau_s = mu_tau +
                                      sum_j L_Dj eps_sj is correlated with w_s; the same for the two models below
    GammaReparamSVI                   eps [S, D + 1]:  the same transform, tau = log alpha (bsc_gamma_predict_pass)
    WeibullReparamSVI                 eps [S, D + 1]:  the same transform, tau = log k (bsc_weibull_predict_pass; y is
                                      the signed response of svi/glm_weibull.py, negative = right-censored, and the
                                      lpd of such a row is its log predictive survival probability; with ``upper``,
                                      bsc_weibull_predict_pass_interval and the log probability of the interval)
    BetaReparamSVI                    eps [S, D + 1]:  the same transform, tau = log phi, the precision
                                      (bsc_beta_predict_pass; the link is a logit: offset allowed, exposure refused)
    LogNormalReparamSVI               eps [S, D + 1]:  the same transform, tau = log(1 / sigma), the inverse scale
                                      (bsc_lognormal_predict_pass; y is the signed response as for the Weibull model;
                                      offset allowed, exposure, upper= and groups= refused)
    ZIPoissonReparamSVI               eps [S, D + 1]:  the same transform, tau = log omega, the log odds of a structural
                                      zero (bsc_zip_predict_pass; a log link: offset or exposure; upper= and groups=
                                      refused)
    StudentTReparamSVI                eps [S, D + 1]:  the same transform, tau = log(1 / sigma), the inverse scale
                                      (bsc_studentt_predict_pass, which also takes the model's df; ``mean`` is the
                                      location -- the mean for df > 1, the median always --, ``var`` +inf for df <= 2;
                                      offset allowed, exposure, upper= and groups= refused)
    HierNegBin/Gamma/WeibullReparamSVI  eps [S, D + J + 3]: the transform below over z = [w | b | zeta | tau], b_new
                                      from the last column; returned as (W, Bt, logtau float32 [S])
                                      (bsc_scalar_predict_pass_groups)
    HierGLMReparamSVI                 eps [S, D + J + 2]:  z = m + e^rho eps[:, :D + J + 1] over z = [w | b | zeta], and
                                      b_new = e^{-zeta / 2} eps[:, D + J + 1], the intercept of a group that was not
                                      seen in training; returned as (W [S, D], Bt [J + 1, ldb]) with Bt[j, s] = b_s[j],
                                      row J = b_new, ldb = 16 ceil(S / 16), padding zero (bsc_predict_pass_groups)
    OrdinalReparamSVI                 eps [S, D + K - 1]:  the two GLM transforms at width P = D + K - 1 over
                                      z = [w | theta], returned whole as Z [S, P] (predict() below hands over to its
                                      predict(): bsc_ordinal_predict_pass, prob [B, K] instead of mean and var)
xi = log s2 is the log-variance of the Gaussian likelihood (``logvar`` of the pass); tau = log phi is the log-dispersion
of the negative binomial, or the log-shape of the Gamma model, and travels in the same slot of the returned pair.

Offsets and weights (logistic, Poisson, negative-binomial, Gamma and Weibull models): ``offset`` (or, with a log link, ``exposure`` = e^offset) is added to the
linear predictor in the pass (bsc_predict_pass_offset), so a Poisson ``mean`` is the expected count at that exposure.
The Beta model takes ``offset`` and ``weights`` the same way and, its link being a logit, no ``exposure``; so does the
log-normal model, whose linear predictor is the location of log t.  The zero-inflated Poisson model follows the Poisson
rules (offset or exposure): its ``mean`` is (1 - pi) times the expected count at that exposure.
A model fitted with an offset refuses to predict without one.  ``weights`` leave every per-row output alone and make
``lpd_sum`` the weighted sum_n v_n lpd_n (float64, on the device, from the lpd vector).

Groups (HierGLMReparamSVI): ``groups`` is one int32 id per row, in [0, J) for a group of the training data or -1 for a
group that was not seen in training; the ids are range-checked once per call (bsc_group_ids_check, one
synchronisation) and the pass adds b_s[g_n] to the linear predictor.  A row with id -1 has its intercept integrated
over N(0, e^{-zeta}) under q(zeta): one draw b_new,s per posterior draw, SHARED by all such rows of the call.  Each
row's ``mean``, ``var`` and ``lpd`` are correct Monte-Carlo estimates of its marginal predictive; JOINT statements about
two rows of the same new group are not (one call cannot tell two new groups apart, and ``lpd_sum`` adds the rows'
marginal log densities, as it does for every model here).  offset, exposure and weights behave as for GLMReparamSVI.
"""
from collections import namedtuple

import numpy as np
import torch

from ._obs import batch_obs, check_link
from ._reparam_base import first_draw, float_batch

# include/bayesic_hip.h: BSC_PREDICT_*
FAMILIES = {"gaussian": 0, "logistic": 1, "poisson": 2}
# One row per family (csrc/bsc_families.h holds the device side of each):
#   entry    its own entry point (the offset may be None), or None: bsc_predict_pass[_offset] with its FAMILIES id
#   link     "log" or "logit": the offset / exposure rules (a logit link takes offset and refuses exposure); "location":
#            the location of log t (of y itself for the Student-t family), offset allowed and exposure refused as for a
#            logit; "count": the log mean of the Poisson part of a mixture, the rules of "log" under a word of its own
#            (the views below keep their contents); None: neither
#   scalar   a per-draw log-scalar rides behind the weights
#   grouped  include/bayesic_hip.h: BSC_SCALAR_*, its id with groups (svi/hier_scalar.py), or None: not built
Family = namedtuple("Family", "entry link scalar grouped")
FAMILY_TABLE = {
    "gaussian": Family(None, None, True, None),
    "logistic": Family(None, "logit", False, None),
    "poisson": Family(None, "log", False, None),
    "negbin": Family("bsc_nb_predict_pass", "log", True, 0),
    "gamma": Family("bsc_gamma_predict_pass", "log", True, 1),
    "weibull": Family("bsc_weibull_predict_pass", "log", True, 2),
    "beta": Family("bsc_beta_predict_pass", "logit", True, None),
    "lognormal": Family("bsc_lognormal_predict_pass", "location", True, None),
    "zip": Family("bsc_zip_predict_pass", "count", True, None),
    "studentt": Family("bsc_studentt_predict_pass", "location", True, None),
}
NO_FAMILY = Family(None, None, False, None)      # softmax and ordinal: their own passes and their own rules
# the table's columns under their earlier names
SCALAR_PASSES = {f: r.entry for f, r in FAMILY_TABLE.items() if r.entry and r.link == "log"}
LOGIT_SCALAR_PASSES = {f: r.entry for f, r in FAMILY_TABLE.items() if r.entry and r.link == "logit"}
SCALAR_FAMILIES = {f: r.grouped for f, r in FAMILY_TABLE.items() if r.grouped is not None}
PREDICT_STREAM = 2     # Philox stream of the predictive draws
MAX_SAMPLES = 64       # draws per bsc_predict_pass call

__all__ = ["posterior_draws", "predict", "heldout_lpd", "family_of", "PREDICT_STREAM", "MAX_SAMPLES"]


def family_of(model):
    """The likelihood family of a driver: its GLM link ("negbin" for NegBinReparamSVI, "gamma" for GammaReparamSVI,
    "weibull" for WeibullReparamSVI, "beta" for BetaReparamSVI, "lognormal" for LogNormalReparamSVI, "zip" for
    ZIPoissonReparamSVI, "studentt" for StudentTReparamSVI, "ordinal" for OrdinalReparamSVI; HierGLMReparamSVI's link
    too -- ``grouped`` tells that model apart), "softmax" for SoftmaxReparamSVI, or "gaussian" for BLRReparamSVI."""
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


def grouped(model):
    """Whether the model is the random-intercept one (svi/hier_glm.py): its predictive takes ``groups=``."""
    return getattr(model, "J", None) is not None and hasattr(model, "_checked_groups")


def table_ld(S):
    """Leading dimension of the intercept table Bt for S draws: whole accumulator chunks of sixteen."""
    return 16 * ((int(S) + 15) // 16)


def intercept_table(b, b_new):
    """Bt float32 [J + 1, ldb] (host) from b [S, J] and b_new [S]: Bt[j, s] = b[s, j], row J = b_new, padding zero."""
    S, J = b.shape
    Bt = np.zeros((J + 1, table_ld(S)), np.float32)
    Bt[:J, :S] = b.T
    Bt[J, :S] = b_new
    return Bt


def _check_samples(n_samples):
    S = int(n_samples)
    if S > MAX_SAMPLES:
        raise ValueError("n_samples=%d: one predictive pass takes at most %d draws" % (S, MAX_SAMPLES))
    if S < 1:
        raise ValueError("n_samples must be at least 1")
    return S


def posterior_draws(model, n_samples=64, seed=None):
    """(W float32 [S, D] on the device, logvar float32 [S] or None) from the model's current q; W is [S, K, D] for
    SoftmaxReparamSVI (its guide is over the K D entries, flattened p = k D + d) and Z [S, D + K - 1] = [w | theta] for
    OrdinalReparamSVI; for NegBinReparamSVI the second
    entry is logphi float32 [S], for GammaReparamSVI and WeibullReparamSVI logshape float32 [S], for BetaReparamSVI
    logprec float32 [S], for LogNormalReparamSVI and StudentTReparamSVI loginvscale float32 [S], for
    ZIPoissonReparamSVI logodds float32 [S]; for HierGLMReparamSVI it is the intercept
    table Bt float32 [J + 1, ldb] (module
    docstring), and for the drivers of svi/hier_scalar.py the triple (W, Bt, logtau float32 [S])."""
    S = _check_samples(n_samples)
    family = family_of(model)
    row = FAMILY_TABLE.get(family, NO_FAMILY)
    ctx, D = model.ctx, model.D
    if grouped(model):
        J = model.J
        scalar = row.grouped is not None         # svi/hier_scalar.py: tau sits behind zeta
        P = D + J + (2 if scalar else 1)
        seed = model.seed if seed is None else int(seed)
        eps_d = torch.zeros((S, P + 1), dtype=torch.float64, device=ctx.device)
        ctx.call("bsc_philox_normal", seed, PREDICT_STREAM, 0, S, P + 1, eps_d)
        eps = eps_d.cpu().numpy()
        z = first_draw(model.lam.cpu().numpy(), eps[:, :P], P, "diag")
        b_new = np.exp(-0.5 * z[:, D + J]) * eps[:, P]
        W = ctx.to_device(np.ascontiguousarray(z[:, :D], np.float32))
        Bt = ctx.to_device(intercept_table(z[:, D:D + J].astype(np.float32), b_new.astype(np.float32)))
        if scalar:
            return W, Bt, ctx.to_device(np.ascontiguousarray(z[:, P - 1], np.float32))
        return W, Bt
    if family == "softmax":
        D = model.n_classes * model.D          # the guide's width; the transforms below are the GLM ones
    elif family == "ordinal":
        D = model.P                            # z = [w | theta], returned whole: the pass reads both from Z [S, P]
    seed = model.seed if seed is None else int(seed)
    scalar = row.scalar                        # a scalar latent rides behind the weights
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
    row = FAMILY_TABLE.get(family, NO_FAMILY)
    if row.entry and row.link in ("logit", "location"):     # the logistic link's rules, in the model's own words
        if exposure is not None:
            raise ValueError("predict: exposure belongs to the Poisson rate model; the %s model takes offset=" % family)
        return batch_obs(model.ctx, B, offset, weights)
    if row.link is None:
        raise ValueError("predict: offset, exposure and weights are for the logistic and Poisson models, not %s" % family)
    # (its own entry: a log link, "log" or "count")
    check_link("poisson" if row.entry else family, offset, exposure, kept="means")
    return batch_obs(model.ctx, B, offset, weights, exposure)


def _groups(model, groups, B):
    """The checked ids of a batch of B rows (a device tensor or a raw pointer), or None for a model without groups."""
    if not grouped(model):
        if groups is not None:
            raise ValueError("predict: groups= belongs to the random-intercept model (HierGLMReparamSVI)")
        return None
    from .hier_glm import check_predict_groups
    check_predict_groups(groups, B)
    g = model._checked_groups(groups, B)
    model.ctx.call("bsc_group_ids_check", g, B, model.J, 1)      # [-1, J): one synchronisation per call
    return g


def predict(model, X, y=None, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None,
            groups=None, upper=None):
    """Posterior predictive of ``model`` for the rows of X: a dict of device tensors ``mean`` and ``var`` (float32
    [B]) and, with y, ``lpd`` (float32 [B]) and ``lpd_sum`` (float64 [1]).  ``draws`` = (W, logvar) reuses draws of
    ``posterior_draws``; otherwise n_samples (at most 64) are drawn with ``seed`` (default: the model's).
    ``offset`` / ``exposure`` / ``weights``: float32 [B] (module docstring); with weights ``lpd_sum`` is the weighted
    sum and ``weight_sum`` (float64 [1]) is sum_n v_n.
    ``groups`` (HierGLMReparamSVI, required there): int32 [B] -- a device tensor, a host array (uploaded) or a raw
    device pointer -- with -1 for a group that was not seen in training.  Such a row's intercept is integrated over
    N(0, e^{-zeta}) with ONE draw per posterior draw that all -1 rows of the call share: per-row ``mean``, ``var`` and
    ``lpd`` are correct Monte-Carlo estimates, joint statements about two rows of the same new group are not.
    ``upper`` (WeibullReparamSVI only): the rows' upper ends in the DEVICE encoding of svi/glm_weibull.pack_censored,
    float32 [B] next to the signed y -- the driver's own predict() takes the plain ones and packs them; ``lpd`` of an
    interval or left-censored row is the log of its predictive probability (bsc_weibull_predict_pass_interval)."""
    family = family_of(model)
    if upper is not None and grouped(model):
        raise NotImplementedError("predict: upper= together with groups is not built (svi/hier_scalar.py)")
    if upper is not None and family != "weibull":
        raise ValueError("predict: upper= (interval and left censoring) belongs to the Weibull model, not %s" % family)
    if family == "softmax":      # its own pass and outputs (prob [B, K] instead of mean and var)
        if groups is not None:
            raise ValueError("predict: groups= belongs to the random-intercept model (HierGLMReparamSVI)")
        return model.predict(X, y, n_samples=n_samples, seed=seed, draws=draws)
    if family == "ordinal":      # its own pass and outputs as well; offset and weights are its predict()'s
        if groups is not None:
            raise ValueError("predict: groups= belongs to the random-intercept model (HierGLMReparamSVI)")
        if exposure is not None:
            raise ValueError("predict: exposure belongs to the Poisson rate model; the ordinal model takes offset=")
        return model.predict(X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, weights=weights)
    groups = _groups(model, groups, int(X.shape[0]))
    offset, weights = _obs(model, family, int(X.shape[0]), offset, exposure, weights)
    if draws is None:
        draws = posterior_draws(model, n_samples, seed)
    row = FAMILY_TABLE.get(family, NO_FAMILY)
    logtau = None
    if groups is not None and row.grouped is not None:       # svi/hier_scalar.py: (W, Bt, logtau [S])
        if len(draws) != 3:
            raise ValueError("draws of a random-intercept model with a learned scalar are (W [S, D], Bt float32 "
                             "[J + 1, ldb], logtau float32 [S]) as posterior_draws returns them")
        W, logvar, logtau = draws
    else:
        W, logvar = draws
    S = _check_samples(W.shape[0])
    X, y = _data(model, X, y)
    ctx = model.ctx
    B = int(X.shape[0])
    if upper is not None:
        if y is None:
            raise ValueError("predict: upper= needs y")
        from ._obs import obs_vector
        upper = obs_vector(ctx, "upper", upper, B)
    ldx = int(X.stride(0)) if B > 1 else max(int(X.stride(0)), model.D)
    dev = ctx.device
    out = {"mean": torch.empty(B, dtype=torch.float32, device=dev),
           "var": torch.empty(B, dtype=torch.float32, device=dev)}
    if y is not None:
        out["lpd"] = torch.empty(B, dtype=torch.float32, device=dev)
        if weights is None:        # (the weighted sum is formed from the lpd vector below)
            out["lpd_sum"] = torch.zeros(1, dtype=torch.float64, device=dev)
    if groups is not None:       # the random-intercept model: `logvar` is the intercept table; the offset may be None
        Bt = logvar
        if Bt.dim() != 2 or Bt.shape[0] != model.J + 1 or Bt.stride(1) != 1 or Bt.dtype != torch.float32:
            raise ValueError("draws of the random-intercept model are (W [S, D], Bt float32 [J + 1, ldb]) as "
                             "posterior_draws returns them")
        if logtau is not None:
            ctx.call("bsc_scalar_predict_pass_groups", row.grouped, X, ldx, y, offset, groups, B, model.D,
                     model.J, W, Bt, int(Bt.stride(0)), logtau, S, out["mean"], out["var"], out.get("lpd"),
                     out.get("lpd_sum"))
        else:
            ctx.call("bsc_predict_pass_groups", FAMILIES[family], X, ldx, y, offset, groups, B, model.D, model.J, W,
                     Bt, int(Bt.stride(0)), S, out["mean"], out["var"], out.get("lpd"), out.get("lpd_sum"))
    elif upper is not None:        # the Weibull model with interval and left censoring; the offset may be None
        ctx.call("bsc_weibull_predict_pass_interval", X, ldx, y, upper, offset, B, model.D, W, logvar, S, out["mean"],
                 out["var"], out.get("lpd"), out.get("lpd_sum"))
    elif family == "studentt":     # its own entry point and the model's degrees of freedom; the offset may be None
        ctx.call(row.entry, X, ldx, y, offset, B, model.D, W, logvar, S, float(model.df), out["mean"], out["var"],
                 out.get("lpd"), out.get("lpd_sum"))
    elif row.entry:                # its own entry point, behind a log or a logit link; the offset may be None
        ctx.call(row.entry, X, ldx, y, offset, B, model.D, W, logvar, S, out["mean"], out["var"], out.get("lpd"),
                 out.get("lpd_sum"))
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


def heldout_lpd(model, X, y, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None,
                groups=None, upper=None):
    """Mean log predictive density per row of the held-out (X, y): lpd_sum / B, a host float (synchronises).  With
    weights: sum_n v_n lpd_n / sum_n v_n.  ``groups`` and ``upper``: as in ``predict``."""
    out = predict(model, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                  weights=weights, groups=groups, upper=upper)
    if "weight_sum" in out:
        return float(out["lpd_sum"].item()) / float(out["weight_sum"].item())
    return float(out["lpd_sum"].item()) / max(int(out["lpd"].shape[0]), 1)
