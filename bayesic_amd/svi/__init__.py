"""Host-side drivers of the SVI inner loop (one class per BASELINE config)."""

from .glm import GLMReparamSVI  # noqa: E402,F401

__all__ = ["GLMReparamSVI"]
