"""A recording double of bayesic_amd.device.Context for the reparameterised drivers (tests only, CPU, computes nothing).

It writes down ``reserve(n)``, every ``call(name, *args)`` and every function of ``lib`` a driver asks, as JSON-ready
lists: scalars as they are (floats by ``float.hex``), None as None, a tensor as [name, element offset, numel, dtype]
with the name of the constructor input (``name(...)``) or driver attribute whose storage holds it, a raw integer
pointer as the integer, a ctypes array as the list of its entries and a ``ctypes.byref`` result as "byref".  Tensors
are named at ``bind(driver)``, which the test calls after every operation, so that a buffer is named by what owned it
then.  ``bsc_blr_noise`` and ``bsc_philox_normal`` fill their output with seeded normals: the first draw and the
predictive draws, which the drivers make on the host, are then not trivial and ``digest`` pins their bytes.
"""
import ctypes
import hashlib

import numpy as np
import torch

_BYREF = type(ctypes.byref(ctypes.c_int32(0)))


class _Pending:
    """A tensor (or an address inside one) that waits for its name."""

    def __init__(self, tensor=None, address=None):
        self.tensor, self.address = tensor, address


class _Lib:
    """The host-side queries the drivers make of the library itself."""
    bsc_blr_pass_update = None      # (asked for with hasattr: the one-call BLR update exists)

    def __init__(self, trace):
        self._trace = trace

    def bsc_glm_group_plan_size(self, B, J):
        self._trace.append(["lib", "bsc_glm_group_plan_size", int(B), int(J)])
        return 8 + B + J + 1 + 3 * (B + J)

    def bsc_glm_group_workspace_bytes(self, handle, B, J):
        self._trace.append(["lib", "bsc_glm_group_workspace_bytes", handle, int(B), int(J)])
        return 64 * (B + J)


class TraceContext:
    device = torch.device("cpu")
    handle = "handle"

    def __init__(self):
        self.trace = []
        self.lib = _Lib(self.trace)
        self._inputs = []           # (name, tensor) in the order they were named: the first match wins

    # -- what the drivers ask of a context ----------------------------------------------------------------------------
    def info(self):
        return {"cu_count": 256}

    def sync(self):
        pass

    def to_device(self, a, dtype=None):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)

    def reserve(self, nbytes):
        self.trace.append(["reserve", int(nbytes)])

    def call(self, name, *args):
        self.trace.append(["call", name] + [self._record(a) for a in args])
        fill = getattr(self, "_" + name, None)
        if fill is not None:
            fill(*args)

    # -- the entry points that are given something to do -----------------------------------------------------------
    @staticmethod
    def _normals(key, out):
        out.copy_(torch.from_numpy(np.random.default_rng(key).standard_normal(tuple(out.shape))))

    def _bsc_blr_noise(self, D, S, seed, step0, n_steps, eps):
        self._normals([seed, 0, step0], eps)

    def _bsc_philox_normal(self, seed, stream, step, S, P, out):
        self._normals([seed, stream, step], out)

    def _bsc_blr_pass_count(self, y, D, S, n):
        n._obj.value = (S + 7) // 8

    def _bsc_glm_group_plan(self, g, B, J, plan, n_seg):
        n_seg._obj.value = J

    # -- recording ----------------------------------------------------------------------------------------------------
    def _record(self, a):
        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, (int, np.integer)):
            return int(a)
        if isinstance(a, (float, np.floating)):
            return float(a).hex()
        if isinstance(a, torch.Tensor):
            return _Pending(tensor=a)
        if isinstance(a, _BYREF):
            return "byref"
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return [_Pending(address=v) for v in a]
            return [self._record(v) for v in a]
        raise TypeError("the recorder does not know how to write down %r" % (a,))

    def name(self, **tensors):
        """Name constructor and set_batch inputs (a name given earlier keeps the storage it was given for)."""
        self._inputs.extend(tensors.items())

    def digest(self, label, tensor):
        self.trace.append(["sha256", label, hashlib.sha256(tensor.contiguous().numpy().tobytes()).hexdigest()])

    def bind(self, driver):
        """Name every tensor recorded since the last bind: a named input first, else the largest tensor attribute of
        the driver on the same storage (the first by name among equals), else "<temporary>"."""
        attrs = sorted(((k, v) for k, v in vars(driver).items() if isinstance(v, torch.Tensor)),
                       key=lambda kv: (-kv[1].numel(), kv[0]))
        owners = self._inputs + attrs

        def resolve(p):
            if p.tensor is not None:
                t = p.tensor
                base = t.untyped_storage().data_ptr()
                for name, o in owners:
                    if o.untyped_storage().data_ptr() == base:
                        return [name, int(t.storage_offset()), int(t.numel()), str(t.dtype)]
                return ["<temporary>", int(t.storage_offset()), int(t.numel()), str(t.dtype)]
            for name, o in owners:
                s = o.untyped_storage()
                if s.data_ptr() <= p.address < s.data_ptr() + s.nbytes():
                    return [name, (p.address - s.data_ptr()) // o.element_size(), None, str(o.dtype)]
            return ["<address>", None, None, None]

        def walk(v):
            if isinstance(v, _Pending):
                return resolve(v)
            return [walk(e) for e in v] if isinstance(v, list) else v

        self.trace[:] = [walk(event) for event in self.trace]
