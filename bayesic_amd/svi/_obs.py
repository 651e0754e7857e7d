"""Offsets, exposure and row weights of the logistic / Poisson models: the argument checks, the checked vectors of a
batch and the drivers' batch state, for svi/glm.py, svi/hier_glm.py and svi/predict.py."""
import torch

# include/bayesic_hip.h: BSC_GLM_*
LINKS = {"logistic": 0, "poisson": 1}


def check_link(link, offset, exposure, kept="is stored as"):
    """The checks of link=, offset= and exposure= that need no device (``kept``: the caller's word for what becomes of
    an exposure)."""
    if link not in LINKS:
        raise ValueError("link must be 'logistic' or 'poisson', got %r" % (link,))
    if exposure is not None and link != "poisson":
        raise ValueError("exposure belongs to the Poisson rate model; link=%r takes offset=" % (link,))
    if exposure is not None and offset is not None:
        raise ValueError("exposure and offset are mutually exclusive (exposure %s offset = log(exposure))" % kept)


def obs_vector(ctx, name, v, rows, log=False):
    """``v`` (offset, weights or exposure; a tensor or a host array) as a float32 [rows] contiguous device tensor,
    checked like y, or None; ``log``: an exposure, returned as its logarithm (computed once, on the device)."""
    if v is None:
        return None
    if not isinstance(v, torch.Tensor):
        v = ctx.to_device(v, torch.float32)
    if v.dtype != torch.float32:
        raise TypeError("%s must be float32" % name)
    if v.dim() != 1 or v.shape[0] != rows:
        raise ValueError("%s must be [%d], one entry per row of X" % (name, rows))
    if rows > 1 and v.stride(0) != 1:
        raise ValueError("%s must be contiguous" % name)
    if log:
        if not bool((v > 0).all() & torch.isfinite(v).all()):
            raise ValueError("exposure must be finite and strictly positive")
        v = torch.log(v)
    return v


def checked_weights(v):
    """The weights' check, finite and >= 0: one synchronisation, so it sits outside step()."""
    if v is not None and not bool((torch.isfinite(v) & (v >= 0)).all()):
        raise ValueError("weights must be finite and >= 0")
    return v


def batch_obs(ctx, rows, offset, weights, exposure=None):
    """(offset or, without one, log exposure; checked weights) of a batch of ``rows`` rows."""
    o = obs_vector(ctx, "exposure" if offset is None else "offset", exposure if offset is None else offset, rows,
                   log=offset is None)
    return o, checked_weights(obs_vector(ctx, "weights", weights, rows))


class ObsBatch:
    """The offset and the weights of a driver's current batch: tensors, raw device pointers or None."""

    def _set_obs(self, offset, weights):
        tensor = lambda v: v if isinstance(v, torch.Tensor) else None
        self.offset, self.weights = tensor(offset), tensor(weights)
        self._oarg = offset if offset is None or isinstance(offset, torch.Tensor) else int(offset)
        self._varg = weights if weights is None or isinstance(weights, torch.Tensor) else int(weights)
