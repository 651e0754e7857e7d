"""BASELINE configurations written on the plugin surface -- Distribution nodes
(bayesic/distribution/base.py:9-172) and ``bayesic.algebra`` expressions -- for the general engines
(``ReparamVI``, ``ScoreFunctionVI``, ``MeanFieldVMP``).  Nothing here names a kernel: which launches an
update turns into is the engines' business (``inference/recognise.py``).
"""
from .. import algebra as A
from ..distribution import InverseGamma, Normal


def linear_regression_log_joint(n_total_over_batch=1.0, alpha0=1.0, beta0=1.0, dtype="float32"):
    """Config 2: y_n ~ N(x_n . w, s2), w | s2 ~ N(0, s2 I), s2 ~ InvGamma(alpha0, beta0),
    with a leading Monte-Carlo sample axis on the latents ``W`` [S, D] and ``xi`` = log s2 [S, 1]:

        log p(y, w, xi) = scale * sum_n log N(y_n | x_n . w, e^xi) + sum_d log N(w_d | 0, e^xi)
                          + log InvGamma(e^xi | alpha0, beta0) + xi          (the Jacobian of s2 = e^xi)

    each density through the node's three-term decomposition (data term + interaction term - log-normaliser,
    bayesic/distribution/base.py:47-69).  Returns (log-joint [S], [(W, D) ...] is the caller's: the latent
    vars ``W`` and ``xi`` and the data vars ``X`` [N, D], ``y`` [N])."""
    X, y = A.var("X", 2, dtype), A.var("y", 1, dtype)
    W, xi = A.var("W", 2, dtype), A.var("xi", 2, dtype)
    x = A.sum(xi, axis=1)                                   # [S]
    s2 = A.exp(x)
    s2_rows = A.dimshuffle(s2, 0, "x")                      # [S, 1]: one variance per draw, broadcast along the data
    likelihood = A.sum(Normal().log_likelihood(A.dimshuffle(y, "x", 0), mean=A.dot(W, X.T), variance=s2_rows),
                       axis=1) * float(n_total_over_batch)
    prior_w = A.sum(Normal().log_likelihood(W, mean=0.0, variance=s2_rows), axis=1)
    prior_xi = InverseGamma().log_likelihood(s2, shape=float(alpha0), scale=float(beta0)) + x
    return likelihood + prior_w + prior_xi, dict(X=X, y=y, W=W, xi=xi)


def _glm_log_joint(link, n_total_over_batch, prior_precision, dtype, offset=False, weights=False):
    import math
    X, y, W = A.var("X", 2, dtype), A.var("y", 1, dtype), A.var("W", 2, dtype)
    names = dict(X=X, y=y, W=W)
    logits = A.dot(W, X.T)                                  # [S, N]
    if offset:
        names["offset"] = A.var("offset", 1, dtype)
        logits = logits + A.dimshuffle(names["offset"], "x", 0)
    log_partition = A.log(1.0 + A.exp(logits)) if link == "logistic" else A.exp(logits)
    rows = A.dimshuffle(y, "x", 0) * logits - log_partition
    if weights:
        names["weights"] = A.var("weights", 1, dtype)
        rows = A.dimshuffle(names["weights"], "x", 0) * rows
    likelihood = A.sum(rows, axis=1) * float(n_total_over_batch)
    tau = float(prior_precision)
    prior_w = A.sum(W * W, axis=1) * (-0.5 * tau) + A.shape(W, 1) * (0.5 * math.log(tau / (2.0 * math.pi)))
    return likelihood + prior_w, names


def logistic_regression_log_joint(n_total_over_batch=1.0, prior_precision=1.0, dtype="float32", offset=False,
                                  weights=False):
    """Bernoulli-logit regression: y_n ~ Bernoulli(sigmoid(x_n . w)), w ~ N(0, I / prior_precision), with a leading
    Monte-Carlo sample axis on the latent ``W`` [S, D]:

        log p(y, w) = scale * sum_n [y_n l_n - log(1 + exp(l_n))] + sum_d log N(w_d | 0, 1 / prior_precision),   l = X w

    (an intercept is a column of ones in X).  ``offset`` / ``weights``: the 1-D data vars ``offset`` and ``weights``
    [N] enter as l = X w + offset and sum_n weights_n [...] (aggregated binomial rows: y = k / n, weights = n); the
    defaults build the expression above.  Returns (log-joint [S], the vars ``X`` [N, D], ``y`` [N], ``W`` and those)."""
    return _glm_log_joint("logistic", n_total_over_batch, prior_precision, dtype, offset, weights)


def poisson_regression_log_joint(n_total_over_batch=1.0, prior_precision=1.0, dtype="float32", offset=False,
                                 weights=False):
    """Poisson regression with the log link: y_n ~ Poisson(exp(x_n . w)), w ~ N(0, I / prior_precision):

        log p(y, w) = scale * sum_n [y_n l_n - exp(l_n)] + sum_d log N(w_d | 0, 1 / prior_precision),   l = X w

    without the term -scale * sum_n lnGamma(y_n + 1), which depends on no latent.  ``offset`` is the rate model's
    log exposure.  Same arguments and return as ``logistic_regression_log_joint``."""
    return _glm_log_joint("poisson", n_total_over_batch, prior_precision, dtype, offset, weights)
