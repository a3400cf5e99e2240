"""Host-side engine object: owns one C-ABI ctx on one GPU and the torch-allocated device
buffers handed to it.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import collections
import ctypes as ct
import hashlib

import numpy as np
import torch

try:  # fast content hash for large host-side matrices (offline wheelhouse); hashlib otherwise
    import xxhash
except ImportError:  # pragma: no cover
    xxhash = None

from . import _lib
from .targets import Target


# Host arrays are keyed by their FULL content at any size (the reference re-reads the matrix on every call, so an
# in-place edit must be seen).  `SAMPLED_HASH_ABOVE` (bytes; None = never) is an explicit opt-in for callers who
# promise not to edit large arrays in place: above it only a strided sample is hashed.
SAMPLED_HASH_ABOVE = None
_WARN_HOST_BYTES = 64 << 20
_warned_big_host_array = False


def _digest(buf):
    if xxhash is not None:
        return xxhash.xxh3_128_hexdigest(buf)
    return hashlib.blake2b(buf, digest_size=16).hexdigest()


def _content_key(arr: np.ndarray):
    """Key a host array by CONTENT: numpy inputs may be edited in place between calls (the
    reference re-reads the matrix on every call), so neither id() nor a sample of the elements may
    hit the cache.  The whole array is hashed (xxh3: ~10 GB/s, i.e. ~0.1 s for the 800 MB matrix of
    D = 1e4 -- once per step() call; a warning says once that a torch tensor on the device, keyed by
    identity and version counter, avoids both the hashing and the upload).  With the module-level
    opt-in ``SAMPLED_HASH_ABOVE`` set, larger arrays are keyed by shape plus the hashes of a 1/256
    strided sample and of the first and last MB (then an in-place edit that misses the sample needs
    ``force=True``)."""
    global _warned_big_host_array
    a = np.ascontiguousarray(arr)
    buf = memoryview(a).cast("B")
    if a.nbytes > _WARN_HOST_BYTES and not _warned_big_host_array:
        _warned_big_host_array = True
        import warnings
        warnings.warn(f"aehmc_amd: a {a.nbytes >> 20} MB host array is hashed on every call and re-uploaded when it "
                      "changes; pass a torch tensor on the device to skip both", stacklevel=4)
    if SAMPLED_HASH_ABOVE is None or a.nbytes <= SAMPLED_HASH_ABOVE:
        return _digest(buf)
    flat = a.reshape(-1)
    sample = np.ascontiguousarray(flat[::256])
    mb = (1 << 20) // a.itemsize
    return ("sampled", a.shape, _digest(memoryview(sample).cast("B")), _digest(memoryview(flat[:mb]).cast("B")),
            _digest(memoryview(flat[-mb:]).cast("B")))


def _param_key(v):
    """Cache key of one target / metric parameter: DEVICE tensors by identity + version counter, anything
    else (CPU tensors, numpy arrays, lists, scalars) by content.  (A CPU tensor can be edited through a numpy view of
    its storage without its version counter moving -- `t.numpy()[0] = 1.0` -- so identity + version is not a safe key
    for it; it is uploaded anyway, hashing it is the cheaper part.)"""
    if isinstance(v, torch.Tensor):
        if v.device.type == "cpu":
            arr = v.detach().to(torch.float64).numpy()
            return ("c", arr.shape, _content_key(arr))
        return ("t", id(v), v._version, tuple(v.shape))
    arr = np.asarray(v, dtype=np.float64)
    return ("n", arr.shape, _content_key(arr))


def _asymmetry(t: torch.Tensor) -> float:
    """max |t - t^T| in row blocks (no D x D temporary)."""
    worst, D = 0.0, t.shape[0]
    for lo in range(0, D, 1024):
        hi = min(D, lo + 1024)
        worst = max(worst, float((t[lo:hi] - t[:, lo:hi].T).abs().max()))
    return worst


def _dev_f64(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=device)


class EngineError(RuntimeError):
    pass


class PerChain:
    """Marks a step size [C] or a diagonal inverse mass matrix [C] / [C, D] as holding one
    value (row) per chain -- what per-chain window adaptation produces.  The reference has
    no chain axis, so a plain [C, D] array would be ambiguous with a dense [D, D] matrix."""

    def __init__(self, value, sqrt_mass=None):
        self.value = value
        self.sqrt_mass = sqrt_mass


class Engine:
    """One aehmc_ctx.  Not thread-safe (as the C-ABI)."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise EngineError("aehmc_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                              "there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.lib = _lib.load()
        ctx = ct.c_void_p()
        rc = self.lib.aehmc_create(ct.byref(ctx), self.device.index or 0)
        self.ctx = ctx
        if rc:
            raise EngineError(f"aehmc_create failed: {self._err()}")
        self._target_key = None
        self._metric_key = None
        self.rtc_cache_dir = self._rtc_cache_dir()
        if self.rtc_cache_dir:
            self._check(self.lib.aehmc_set_rtc_cache(self.ctx, self.rtc_cache_dir.encode()), "aehmc_set_rtc_cache")
        # metric handles: (device imm, device sqrt-mass) per metric content, so that kernels which alternate between
        # metrics on one device (each kernel its own dense mass matrix) factor every matrix ONCE
        self._metric_cache = collections.OrderedDict()
        self.metric_cache_bytes = 4 << 30
        self.n_metric_factorizations = 0
        self._keep = {}
        self._ws = None
        self.D = None
        self.metric_ndim = None
        self.metric_D = None

    @staticmethod
    def _rtc_cache_dir():
        """Where the compiled code objects of user-defined targets are kept across processes: AEHMC_AMD_RTC_CACHE (a
        directory; "0" / "" = off), default ~/.cache/aehmc_amd/rtc-<hash of the library's sources> -- the headers a
        run-time compiled program includes are part of what it was compiled from."""
        import os
        from . import _build
        where = os.environ.get("AEHMC_AMD_RTC_CACHE")
        if where is not None and where in ("", "0"):
            return None
        try:
            base = where or os.path.join(os.path.expanduser("~"), ".cache", "aehmc_amd")
            path = os.path.join(base, "rtc-" + _build.source_hash()[:16])
            os.makedirs(path, exist_ok=True)
            return path
        except OSError:
            return None

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.aehmc_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    def _err(self):
        return self.lib.aehmc_last_error(self.ctx).decode()

    def _check(self, rc, what):
        if rc:
            raise EngineError(f"{what} failed ({rc}): {self._err()}")

    @property
    def stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ binding
    def set_target(self, target, D: int, force: bool = False, scalar=None):
        # a Python function of the position (the reference's logprob_fn): traced once into a Custom / CustomJoint target
        if not isinstance(target, Target):
            from . import targets as _targets
            target = _targets.as_target(target, D, scalar)
        # keyed by the CONTENT of the parameters (numpy arrays edited in place between calls must be seen,
        # as for the metric below), not by the identity of the Target object
        params = target.params()
        key = (type(target), D, tuple((k, _param_key(v)) for k, v in sorted(params.items())))
        if getattr(target, "source", None) is not None:
            key = key + (target.source,)
        if self._target_key == key and not force:
            return
        if target.dim is not None and target.dim != D:
            raise ValueError(f"target has dimension {target.dim}, position has {D}")
        p = {k: _dev_f64(v, self.device) for k, v in params.items()}
        if getattr(target, "source", None) is not None:  # user-defined coordinate-wise target: compiled with hipRTC
            import os
            arrs = [p[f"p{k}"] for k in range(len(target.param_list))]
            ptrs = (ct.c_void_p * max(len(arrs), 1))(*[a.data_ptr() for a in arrs])
            inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
            # a failed compile leaves the ctx bound to what it was bound to (aehmc_set_custom_target is a
            # transaction): the arrays of THAT binding must stay alive, so `_keep` changes only on success
            if "X" in p:  # row-reduction target over a data matrix
                X, y = p["X"].contiguous(), p["y"].reshape(-1).contiguous()
                if X.ndim != 2 or X.shape[1] != D or y.numel() != X.shape[0]:
                    raise ValueError(f"GLM target: X must be [N, {D}] and y [N], got {tuple(X.shape)} and {tuple(y.shape)}")
                keep = (target, p, X, y)
                self._check(self.lib.aehmc_set_custom_glm_target(self.ctx, target.source.encode(), D, X.shape[0],
                                                                 X.data_ptr(), y.data_ptr(), ptrs, len(arrs), inc.encode()),
                            "aehmc_set_custom_glm_target")
            elif target.kind == 7:  # targets.T_JOINT: a joint density, differentiated by the engine (D <= 2048, or 10176 with a reverse-mode program; single-launch kernels up to 64)
                keep = (target, p)
                self._check(self.lib.aehmc_set_custom_joint_target(self.ctx, target.source.encode(), D, ptrs, len(arrs),
                                                                   inc.encode()), "aehmc_set_custom_joint_target")
            else:
                keep = (target, p)
                self._check(self.lib.aehmc_set_custom_target(self.ctx, target.source.encode(), D, ptrs, len(arrs),
                                                             inc.encode()), "aehmc_set_custom_target")
            self._keep["target"] = keep
            self._target_key, self.D = key, D
            self._ws = None
            return
        c = _lib.CTarget(kind=target.kind, D=D, N=0)
        for name in ("mu", "sigma", "prec", "X", "y"):
            if name in p:
                setattr(c, name, p[name].data_ptr())
        if "X" in p:
            c.N = p["X"].numel()
        self._check(self.lib.aehmc_set_target(self.ctx, ct.byref(c)), "aehmc_set_target")
        self._keep["target"] = (target, p)
        # a target of the same kind and size has the workspace layout of the one it replaces: the buffer stays bound, and
        # with it what the engine keeps there (the whitened carry record, which the engine itself drops unless the new
        # arrays hold the old content)
        same_layout = self._target_key is not None and self._target_key[:2] == key[:2] and len(key) == 3
        self._target_key, self.D = key, D
        if not same_layout:
            self._ws = None

    def set_metric(self, inverse_mass_matrix, D: int, force: bool = False, sqrt_mass=None):
        """gaussian_metric(inverse_mass_matrix) -- aehmc/metrics.py:44-63.  ``sqrt_mass``: the caller's own device array
        of sqrt(1 / imm) / L^-T, bound instead of one computed here (pooled window adaptation keeps both up itself)."""
        imm = inverse_mass_matrix
        if isinstance(imm, PerChain):
            return self._set_metric_per_chain(imm, D)
        ndim = imm.ndim if hasattr(imm, "ndim") else np.ndim(imm)
        if ndim > 2:
            raise ValueError(
                f"Expected a mass matrix of dimension 1 (diagonal) or 2, got {ndim}")
        if isinstance(imm, torch.Tensor):
            key = (id(imm), imm._version, D)
        else:  # numpy / python scalars may be mutated in place: keyed by content, whatever the size
            arr = np.asarray(imm, dtype=np.float64)
            key = (arr.shape, _content_key(arr), D)
        if self._metric_key == key and not force:
            return
        handle = None if force else self._metric_cache.get(key)
        if handle is None:
            t = _dev_f64(imm, self.device)
            if ndim == 2:
                if t.shape != (D, D):
                    raise ValueError(f"dense inverse mass matrix must be [{D},{D}], got {tuple(t.shape)}")
                # the reference factors one triangle (metrics.py:56) and multiplies by the full matrix
                # (metrics.py:71); the two agree for a symmetric matrix.  Estimates such as A @ A.T or
                # a Welford covariance are symmetric only up to rounding: tolerate that much.
                if _asymmetry(t) > 1e-10 * float(t.diagonal().abs().max()):
                    raise ValueError("dense inverse mass matrix must be symmetric")
            else:
                t = t.reshape(-1)
                if ndim == 1 and t.numel() != D:
                    raise ValueError(f"diagonal inverse mass matrix must have {D} entries")
            if sqrt_mass is not None:
                sm = sqrt_mass.reshape(t.shape)
            else:  # sqrt(1 / imm) / L^-T (metrics.py:45,49,56-58), once per metric content
                sm = torch.empty_like(t)
                self._check(self.lib.aehmc_metric_sqrt(self.ctx, ndim, D, t.data_ptr(), sm.data_ptr(), self.stream),
                            "aehmc_metric_sqrt")
                self.n_metric_factorizations += 1
            handle = (imm, t, sm)  # (the caller's object too: a torch tensor's id() must stay taken while cached)
            self._metric_cache[key] = handle
            held = 0
            for k in reversed(list(self._metric_cache)):  # keep the most recent handles within the byte budget
                held += 2 * self._metric_cache[k][1].numel() * 8
                if held > self.metric_cache_bytes and k != key:
                    del self._metric_cache[k]
        else:
            self._metric_cache.move_to_end(key)
        _, t, sm = handle
        c = _lib.CMetric(ndim=ndim, D=D, imm=t.data_ptr(), sqrt_mass=sm.data_ptr())
        self._keep["metric"] = handle
        self._check(self.lib.aehmc_set_metric(self.ctx, ct.byref(c)), "aehmc_set_metric")
        if self.metric_ndim != ndim:
            self._ws = None
        self._metric_key, self.metric_ndim, self.metric_D = key, ndim, D

    def _set_metric_per_chain(self, pc: PerChain, D: int):
        t = _dev_f64(pc.value, self.device)
        if t.ndim == 1:      # [C] scalar metrics (scalar positions): ndim 0
            ndim, t = 0, t.reshape(-1, 1)
        elif t.ndim == 2:    # [C, D] diagonal metrics
            ndim = 1
            if t.shape[1] != D:
                raise ValueError(f"per-chain diagonal inverse mass matrix must be [C,{D}]")
        elif t.ndim == 3:    # [C, D, D] dense metrics (is_mass_matrix_full adaptation)
            ndim = 2
            if t.shape[1:] != (D, D):
                raise ValueError(f"per-chain dense inverse mass matrix must be [C,{D},{D}]")
        else:
            raise ValueError("PerChain inverse mass matrix must be [C], [C, D] or [C, D, D]")
        if pc.sqrt_mass is not None:
            sm = _dev_f64(pc.sqrt_mass, self.device).reshape(t.shape)
        elif ndim == 2:      # L^-T per chain (metrics.py:56-58), on the device
            t = t.contiguous()
            # one wavefront factors one matrix: ~25 ms for 4096 matrices of 200 x 200.  A device tensor that has not
            # changed since the last call (identity + version counter) keeps its factors; window adaptation hands
            # sqrt_mass over itself
            key = (id(pc.value), pc.value._version, tuple(t.shape)) if isinstance(pc.value, torch.Tensor) else None
            cached = self._keep.get("pc_sqrt")
            if key is not None and cached is not None and cached[0] == key:
                sm = cached[2]
            else:
                sm = torch.empty_like(t)
                self._check(self.lib.aehmc_metric_sqrt_per_chain(self.ctx, t.shape[0], D, t.data_ptr(),
                                                                 sm.data_ptr(), self.stream),
                            "aehmc_metric_sqrt_per_chain")
                self.n_metric_factorizations += 1
                if key is not None:
                    self._keep["pc_sqrt"] = (key, pc.value, sm)  # (the tensor itself: its id() stays taken while cached)
        else:
            sm = torch.sqrt(torch.reciprocal(t))
        c = _lib.CMetric(ndim=ndim, per_chain=1, D=D, imm=t.data_ptr(), sqrt_mass=sm.data_ptr(),
                         n_chains=t.shape[0])
        self._keep["metric"] = (pc, t, sm)
        self._check(self.lib.aehmc_set_metric(self.ctx, ct.byref(c)), "aehmc_set_metric")
        if self.metric_ndim != ndim:
            self._ws = None
        self._metric_key, self.metric_ndim, self.metric_D = None, ndim, D

    def set_step_sizes(self, eps):
        """eps: PerChain -> per-chain step sizes; anything else -> scalar (returned)."""
        if isinstance(eps, PerChain):
            self._bind_step_sizes(_dev_f64(eps.value, self.device).reshape(-1))
            return 0.0
        self._clear_step_sizes()
        return float(eps)

    def _bind_step_sizes(self, t):
        self._keep["eps"] = t
        self._check(self.lib.aehmc_set_step_sizes(self.ctx, t.data_ptr(), t.numel()), "aehmc_set_step_sizes")

    def _clear_step_sizes(self):
        """Per-chain step sizes apply to ONE step/sample call: the ctx is shared per device and
        must not carry them into an unrelated later call."""
        self._keep.pop("eps", None)
        self._check(self.lib.aehmc_set_step_sizes(self.ctx, None, 0), "aehmc_set_step_sizes")

    def _step_call(self, fn, what, *args):
        try:
            self._check(fn(*args), what)
        finally:  # kernel arguments were captured at launch: safe to drop the binding now
            self._clear_step_sizes()

    def synchronize(self):
        """Wait for the stream and raise on device-side failures that are not data."""
        self._check(self.lib.aehmc_synchronize(self.ctx, self.stream), "aehmc_synchronize")

    def ensure_workspace(self, C: int, max_exp: int):
        need = self.lib.aehmc_workspace_bytes(self.ctx, C, max_exp)
        if need < 0:
            raise EngineError("aehmc_workspace_bytes: target/metric not set")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws_bound = None
            self._ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        # bound once per buffer: aehmc_set_workspace tells the engine that whatever it kept in the workspace is gone
        if getattr(self, "_ws_bound", None) != (self._ws.data_ptr(), self._ws.numel()):
            self._check(self.lib.aehmc_set_workspace(self.ctx, self._ws.data_ptr(), self._ws.numel()),
                        "aehmc_set_workspace")
            self._ws_bound = (self._ws.data_ptr(), self._ws.numel())

    def rtc_stats(self):
        """(programs compiled by hipRTC, programs loaded from the on-disk cache) of this engine's ctx."""
        import ctypes as ct
        a, b = ct.c_int64(0), ct.c_int64(0)
        self._check(self.lib.aehmc_rtc_stats(self.ctx, ct.byref(a), ct.byref(b)), "aehmc_rtc_stats")
        return a.value, b.value

    def set_option(self, name: str, value: int):
        self._check(self.lib.aehmc_set_option(self.ctx, name.encode(), int(value)), "aehmc_set_option")

    def set_white_basis(self, V=None, lam=None):
        """ "dense_eigen": the caller's eigenbasis of the whitened operator H = L^T P L (``V`` [D, D], its columns the
        eigenvectors, ``lam`` [D]) in place of the solver's; ``None`` clears it.  Checked on the device when the next
        NUTS call forms the route; a basis that does not fit is rejected and the whitened route runs."""
        if V is None:
            self._check(self.lib.aehmc_set_white_basis(self.ctx, 0, None, None, self.stream), "aehmc_set_white_basis")
            return
        V, lam = _dev_f64(V, self.device).contiguous(), _dev_f64(lam, self.device).reshape(-1).contiguous()
        D = lam.numel()
        if tuple(V.shape) != (D, D):
            raise ValueError(f"white basis: V must be [{D},{D}], got {tuple(V.shape)}")
        self._check(self.lib.aehmc_set_white_basis(self.ctx, D, V.data_ptr(), lam.data_ptr(), self.stream),
                    "aehmc_set_white_basis")

    def white_basis_info(self):
        """What the last whitened NUTS call decided about the eigen route: dict(state, orth, resid, solver_ms) --
        include/aehmc_hip.h: aehmc_white_basis_info.  state > 0: the route runs."""
        state, orth, resid, ms = ct.c_int32(0), ct.c_double(0), ct.c_double(0), ct.c_double(0)
        self._check(self.lib.aehmc_white_basis_info(self.ctx, ct.byref(state), ct.byref(orth), ct.byref(resid),
                                                    ct.byref(ms)), "aehmc_white_basis_info")
        return dict(state=state.value, orth=orth.value, resid=resid.value, solver_ms=ms.value)

    # ------------------------------------------------------------------ calls
    def new_state(self, q):
        C, D = q.shape
        U = torch.empty(C, dtype=torch.float64, device=self.device)
        g = torch.empty_like(q)
        self._check(self.lib.aehmc_new_state(self.ctx, C, q.data_ptr(), U.data_ptr(), g.data_ptr(),
                                             self.stream), "aehmc_new_state")
        return U, g

    def check_gradient(self, q, rtol=1e-5, max_coordinates=32):
        """A hand-written gradient of a user-defined target against central differences of its own potential, at the
        first chains of ``q`` (the reference differentiates ``logprob_fn`` itself, hmc.py:33-34: there a wrong gradient
        cannot exist; here it would sample the wrong distribution silently).  Raises ValueError."""
        C, D = q.shape
        qs = q[:min(C, 2)].detach()
        self.ensure_workspace(max(C, 2 * min(D, max_coordinates)), 1)  # (the perturbed positions are evaluated as chains)
        U0, g = self.new_state(qs.contiguous())
        gen = np.random.default_rng(12345)
        idx = np.arange(D) if D <= max_coordinates else np.sort(gen.choice(D, max_coordinates, replace=False))
        cols = torch.as_tensor(idx, device=self.device)
        rows = torch.arange(len(idx), device=self.device)
        worst = 0.0
        for c in range(qs.shape[0]):
            h = 1e-6 * torch.clamp(qs[c].abs(), min=1.0)[cols]
            pert = qs[c].repeat(2 * len(idx), 1)
            pert[rows, cols] += h
            pert[rows + len(idx), cols] -= h
            Up, _ = self.new_state(pert.contiguous())
            fd = (Up[:len(idx)] - Up[len(idx):]) / (2 * h)
            ga = g[c][cols]
            # (central differences: truncation of order h^2, rounding of order eps |U| / h)
            tol = rtol * torch.clamp(ga.abs(), min=1.0) + 1e-9 * U0[c].abs() / h
            err = (fd - ga).abs() / tol
            k = int(torch.argmax(err))
            worst = max(worst, float(err[k]))
            if not float(err[k]) <= 1.0:
                raise ValueError(
                    f"user-defined target: the hand-written gradient disagrees with central differences of the potential at "
                    f"coordinate {int(idx[k])} (gradient {float(ga[k]):.9g}, finite difference {float(fd[k]):.9g}); write the "
                    "log-density only (aehmc_logp / aehmc_glm_loglik + aehmc_glm_logprior) and let the engine differentiate it")
        return worst

    def _diag(self, C, D, nuts):
        # every array is fully written by the kernels: no memset launches
        dev = self.device
        i64 = torch.empty(2, C, dtype=torch.int64, device=dev)
        i32 = torch.empty(2, C, dtype=torch.int32, device=dev)
        out = dict(
            momentum=torch.empty(C, D, dtype=torch.float64, device=dev),
            acceptance_probability=torch.empty(C, dtype=torch.float64, device=dev),
            num_doublings=i64[0], is_turning=i32[0], is_diverging=i32[1], n_leapfrog=i64[1])
        c = _lib.CDiagnostics(**{k: v.data_ptr() for k, v in out.items()})
        out["flags"] = i32  # (is_turning, is_diverging) as one array: one conversion to bool for both
        return out, c

    def hmc_step(self, rng, eps, L, thr, q, U, g):
        C, D = q.shape
        self.ensure_workspace(C, 1)
        out, c = self._diag(C, D, False)
        self._step_call(self.lib.aehmc_hmc_step, "aehmc_hmc_step", self.ctx, C, rng.data_ptr(), float(eps),
                        int(L), float(thr), q.data_ptr(), U.data_ptr(), g.data_ptr(), ct.byref(c), self.stream)
        return out

    def _history_buffers(self, n, C, D, keep_samples, into):
        """What a sample() call records per transition: the draws [n, C, D] -- fresh, or the head of the caller's buffer
        ``into`` (summary.run folds chunk after chunk from one buffer); None without ``keep_samples`` -- and the
        acceptance [n, C] and divergence [n, C] histories."""
        if not keep_samples:
            samples = None
        elif into is None:
            samples = torch.empty(n, C, D, dtype=torch.float64, device=self.device)
        elif into.dtype != torch.float64 or into.device != self.device or not into.is_contiguous() or into.numel() < n * C * D:
            raise ValueError(f"samples buffer must be a contiguous float64 tensor on {self.device} with at least "
                             f"{n * C * D} elements")
        else:
            samples = into.reshape(-1)[:n * C * D].reshape(n, C, D)
        return (samples, torch.empty(n, C, dtype=torch.float64, device=self.device),
                torch.empty(n, C, dtype=torch.int32, device=self.device))

    def hmc_sample(self, rng, eps, L, thr, n, q, U, g, keep_samples=True, into=None):
        C, D = q.shape
        self.ensure_workspace(C, 1)
        out, c = self._diag(C, D, False)
        samples, acc, div = self._history_buffers(n, C, D, keep_samples, into)
        self._step_call(
            self.lib.aehmc_hmc_sample, "aehmc_hmc_sample",
            self.ctx, C, rng.data_ptr(), float(eps), int(L), float(thr), int(n), q.data_ptr(),
            U.data_ptr(), g.data_ptr(), ct.byref(c), samples.data_ptr() if keep_samples else None,
            acc.data_ptr(), div.data_ptr(), self.stream)
        out["samples"], out["acceptance_history"], out["divergence_history"] = samples, acc, div
        return out

    def hmc_sample_lengths(self, rng, eps, lengths, thr, q, U, g, keep_samples=True, into=None):
        """``hmc_sample`` with one trajectory length per transition (``lengths``: a list of ints >= 0): one engine
        call -- one launch on the routes whose kernels read the lengths on the device; ``n_leapfrog`` is their sum."""
        C, D = q.shape
        n = len(lengths)
        self.ensure_workspace(C, 1)
        out, c = self._diag(C, D, False)
        samples, acc, div = self._history_buffers(n, C, D, keep_samples, into)
        self._step_call(
            self.lib.aehmc_hmc_sample_lengths, "aehmc_hmc_sample_lengths",
            self.ctx, C, rng.data_ptr(), float(eps), (ct.c_int64 * n)(*lengths), float(thr), n, q.data_ptr(),
            U.data_ptr(), g.data_ptr(), ct.byref(c), samples.data_ptr() if keep_samples else None,
            acc.data_ptr(), div.data_ptr(), self.stream)
        out["samples"], out["acceptance_history"], out["divergence_history"] = samples, acc, div
        return out

    def nuts_step(self, rng, eps, max_exp, thr, q, U, g):
        C, D = q.shape
        self.ensure_workspace(C, max_exp)
        out, c = self._diag(C, D, True)
        self._step_call(self.lib.aehmc_nuts_step, "aehmc_nuts_step", self.ctx, C, rng.data_ptr(), float(eps),
                        int(max_exp), float(thr), q.data_ptr(), U.data_ptr(), g.data_ptr(), ct.byref(c),
                        self.stream)
        return out

    def nuts_sample(self, rng, eps, max_exp, thr, n, q, U, g, keep_samples=True, into=None):
        C, D = q.shape
        self.ensure_workspace(C, max_exp)
        out, c = self._diag(C, D, True)
        samples, acc, div = self._history_buffers(n, C, D, keep_samples, into)
        total = torch.zeros(C, dtype=torch.int64, device=self.device)
        self._step_call(
            self.lib.aehmc_nuts_sample, "aehmc_nuts_sample",
            self.ctx, C, rng.data_ptr(), float(eps), int(max_exp), float(thr), int(n), q.data_ptr(),
            U.data_ptr(), g.data_ptr(), ct.byref(c), samples.data_ptr() if keep_samples else None,
            acc.data_ptr(), div.data_ptr(), total.data_ptr(), self.stream)
        out["samples"], out["acceptance_history"], out["divergence_history"] = samples, acc, div
        out["n_leapfrog"] = total
        return out

    def _warmup(self, nuts, pooled, rng, schedule, target_accept, length, thr, q, U, g, st, cstate, imm):
        """The whole window-adaptation loop around a NUTS (``length``: max_num_expansions) or HMC (``length``:
        num_integration_steps) kernel in one C-ABI call (no Python between warm-up steps).  The adaptation state's own
        arrays are bound as the step sizes and as the metric -- per chain (``imm``: a PerChain), or ``pooled`` the SHARED
        one -- because the update kernels rewrite them in place."""
        C, D = q.shape
        out, c = self._diag(C, D, nuts)
        n = len(schedule)
        stage = (ct.c_int32 * n)(*[int(s) for s, _ in schedule])
        wend = (ct.c_int32 * n)(*[int(bool(e)) for _, e in schedule])
        if pooled:
            self.set_metric(imm, D, force=True, sqrt_mass=st["sqrt_mass"])
        else:
            self.set_metric(imm, D)
        self.ensure_workspace(C, length if nuts else 1)  # (after the metric: a dense one needs more work vectors)
        self._bind_step_sizes(st["step_size"])
        what = f"aehmc_{'nuts' if nuts else 'hmc'}_warmup{'_pooled' if pooled else ''}"
        try:
            self._step_call(getattr(self.lib, what), what, self.ctx, C, rng.data_ptr(), n, stage, wend,
                            float(target_accept), int(length), float(thr), q.data_ptr(), U.data_ptr(), g.data_ptr(),
                            ct.byref(c), ct.byref(cstate), self.stream)
        finally:
            if pooled:
                self.forget_metric()
        return out

    def leapfrog(self, eps, nsteps, q, p, U, g):
        C, D = q.shape
        self.ensure_workspace(C, 1)
        self._check(self.lib.aehmc_leapfrog(self.ctx, C, float(eps), int(nsteps), q.data_ptr(),
                                            p.data_ptr(), U.data_ptr(), g.data_ptr(), self.stream),
                    "aehmc_leapfrog")

    def kinetic_energy(self, p):
        C, D = p.shape
        self.ensure_workspace(C, 1)
        K = torch.empty(C, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_kinetic_energy(self.ctx, C, p.data_ptr(), K.data_ptr(), self.stream),
                    "aehmc_kinetic_energy")
        return K

    def is_turning(self, pl, pr, ps):
        C, D = pl.shape
        self.ensure_workspace(C, 1)
        out = torch.empty(C, dtype=torch.int32, device=self.device)
        self._check(self.lib.aehmc_is_turning(self.ctx, C, pl.data_ptr(), pr.data_ptr(), ps.data_ptr(),
                                              out.data_ptr(), self.stream), "aehmc_is_turning")
        return out.bool()

    def rng_normals(self, rng, n):
        C = rng.shape[0]
        out = torch.empty(C, n, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_rng_normals(self.ctx, C, rng.data_ptr(), n, out.data_ptr(), self.stream),
                    "aehmc_rng_normals")
        return out

    def rng_bernoulli(self, rng, p):
        C, n = p.shape
        out = torch.empty(C, n, dtype=torch.int32, device=self.device)
        self._check(self.lib.aehmc_rng_bernoulli(self.ctx, C, rng.data_ptr(), n, p.data_ptr(),
                                                 out.data_ptr(), self.stream), "aehmc_rng_bernoulli")
        return out

    def gemm_nt(self, A, B):
        M, K = A.shape
        N = B.shape[0]
        out = torch.empty(M, N, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_gemm_nt(self.ctx, M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(),
                                           B.stride(0), out.data_ptr(), out.stride(0), self.stream),
                    "aehmc_gemm_nt")
        return out

    def gemm_nt_tri(self, A, B, tri, row_idx=None, n_rows=None, out=None):
        """A B^T with the triangular hint `tri` on B (0 none, 1 lower, 2 upper; aehmc_gemm_nt_tri); `row_idx` [M] int32
        and `n_rows` [1] int32 (device tensors, both or neither) select the rows that are computed and written."""
        M, K = A.shape
        N = B.shape[0]
        if out is None:
            out = torch.empty(M, N, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_gemm_nt_tri(self.ctx, M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0),
                                               out.data_ptr(), out.stride(0), int(tri),
                                               row_idx.data_ptr() if row_idx is not None else None,
                                               n_rows.data_ptr() if n_rows is not None else None, self.stream),
                    "aehmc_gemm_nt_tri")
        return out

    # ------------------------------------------------------------------ warm-up
    def adapt_alloc(self, C, D, full=False):
        dev, f64, i64 = self.device, torch.float64, torch.int64
        mat = (C, D, D) if full else (C, D)
        st = dict(da_step=torch.empty(C, dtype=i64, device=dev), da_x=torch.empty(C, dtype=f64, device=dev),
                  da_x_avg=torch.empty(C, dtype=f64, device=dev), da_g_avg=torch.empty(C, dtype=f64, device=dev),
                  da_mu=torch.empty(C, dtype=f64, device=dev), wc_mean=torch.empty(C, D, dtype=f64, device=dev),
                  wc_m2=torch.empty(mat, dtype=f64, device=dev), wc_n=torch.empty(C, dtype=i64, device=dev),
                  step_size=torch.empty(C, dtype=f64, device=dev), imm=torch.empty(mat, dtype=f64, device=dev),
                  sqrt_mass=torch.empty(mat, dtype=f64, device=dev))
        if full and D > 64:  # scratch of the window-end factorisation (LDS holds it up to D = 64)
            st["work"] = torch.empty(mat, dtype=f64, device=dev)
        return st, self.adapt_cstate(st, full)

    @staticmethod
    def adapt_cstate(st, full):
        return _lib.CAdaptState(full=int(bool(full)), **{k: v.data_ptr() for k, v in st.items()})

    def adapt_init(self, C, D, initial_step_size, cstate):
        self._check(self.lib.aehmc_adapt_init(self.ctx, C, D, float(initial_step_size), ct.byref(cstate),
                                              self.stream), "aehmc_adapt_init")

    def adapt_update(self, C, D, stage, window_end, last, target, p_accept, position, cstate):
        self._check(self.lib.aehmc_adapt_update(self.ctx, C, D, int(stage), int(window_end), int(last),
                                                float(target), p_accept.data_ptr(), position.data_ptr(),
                                                ct.byref(cstate), self.stream), "aehmc_adapt_update")

    # ------------------------------------------------------------------ pooled warm-up
    def pooled_adapt_alloc(self, C, D, full=False):
        """The state of a pooled adaptation: one dual-averaging state, one Welford state, one metric; step_size [C]."""
        dev, f64, i64 = self.device, torch.float64, torch.int64
        mat = (D, D) if full else (D,)
        st = dict(da_step=torch.empty(1, dtype=i64, device=dev), da_x=torch.empty(1, dtype=f64, device=dev),
                  da_x_avg=torch.empty(1, dtype=f64, device=dev), da_g_avg=torch.empty(1, dtype=f64, device=dev),
                  da_mu=torch.empty(1, dtype=f64, device=dev), wc_mean=torch.empty(D, dtype=f64, device=dev),
                  wc_m2=torch.empty(mat, dtype=f64, device=dev), wc_n=torch.empty(1, dtype=i64, device=dev),
                  step_size=torch.empty(C, dtype=f64, device=dev), imm=torch.empty(mat, dtype=f64, device=dev),
                  sqrt_mass=torch.empty(mat, dtype=f64, device=dev))
        return st, self.pooled_cstate(st, full)

    @staticmethod
    def pooled_cstate(st, full):
        return _lib.CPooledAdaptState(full=int(bool(full)), **{k: v.data_ptr() for k, v in st.items()})

    def pooled_adapt_init(self, C, D, initial_step_size, cstate):
        self._check(self.lib.aehmc_pooled_adapt_init(self.ctx, C, D, float(initial_step_size), ct.byref(cstate),
                                                     self.stream), "aehmc_pooled_adapt_init")

    def pooled_adapt_update(self, C, D, stage, window_end, last, target, p_accept, position, cstate):
        self._check(self.lib.aehmc_pooled_adapt_update(self.ctx, C, D, int(stage), int(window_end), int(last),
                                                       float(target), p_accept.data_ptr(), position.data_ptr(),
                                                       ct.byref(cstate), self.stream), "aehmc_pooled_adapt_update")

    # ------------------------------------------------------------------ ChEES warm-up
    def chees_alloc(self, C, D=None):
        """The state of a ChEES adaptation: every array [1] but step_size [C]; with ``D`` also ``sums`` [3 + 2 D], which
        an update fills with S, A, abar and the column means m0, m1."""
        dev, f64, i64 = self.device, torch.float64, torch.int64
        st = {name: torch.empty(1, dtype=i64 if name in ("step", "num_steps", "da_step") else f64, device=dev)
              for name, _ in _lib.CCheesState._fields_[:-2]}
        st["step_size"] = torch.empty(C, dtype=f64, device=dev)
        if D is not None:
            st["sums"] = torch.empty(3 + 2 * D, dtype=f64, device=dev)
        return st, self.chees_cstate(st)

    @staticmethod
    def chees_cstate(st):
        return _lib.CCheesState(**{k: v.data_ptr() for k, v in st.items()})

    def chees_init(self, C, initial_step_size, initial_trajectory_length, cstate):
        self._check(self.lib.aehmc_chees_init(self.ctx, C, float(initial_step_size), float(initial_trajectory_length),
                                              ct.byref(cstate), self.stream), "aehmc_chees_init")

    def chees_update(self, C, D, last, target, learning_rate, max_num_steps, position_before, position_after, momentum,
                     inverse_mass_diag, inverse_mass_scalar, accepted, p_accept, cstate):
        """``inverse_mass_diag``: a [D] tensor or None (then ``inverse_mass_scalar``); ``accepted``: int32 [C]."""
        self._check(self.lib.aehmc_chees_update(
            self.ctx, C, D, int(last), float(target), float(learning_rate), int(max_num_steps),
            position_before.data_ptr(), position_after.data_ptr(), momentum.data_ptr(),
            inverse_mass_diag.data_ptr() if inverse_mass_diag is not None else None, float(inverse_mass_scalar),
            accepted.data_ptr(), p_accept.data_ptr(), ct.byref(cstate), self.stream), "aehmc_chees_update")

    def chees_warmup(self, rng, n, target, learning_rate, max_num_steps, inverse_mass_scalar, thr, q, U, g, st, cstate):
        """The whole ChEES warm-up in one C-ABI call (``aehmc_chees_warmup``): ``n`` x (transition of the state's own
        ``num_steps``, update).  The metric is bound by the caller; the state's ``step_size`` is bound here."""
        C, D = q.shape
        self.ensure_workspace(C, 1)
        out, c = self._diag(C, D, False)
        self._bind_step_sizes(st["step_size"])
        self._step_call(self.lib.aehmc_chees_warmup, "aehmc_chees_warmup", self.ctx, C, rng.data_ptr(), int(n),
                        float(target), float(learning_rate), int(max_num_steps), float(inverse_mass_scalar), float(thr),
                        q.data_ptr(), U.data_ptr(), g.data_ptr(), ct.byref(c), ct.byref(cstate), self.stream)
        return out

    # ------------------------------------------------------------------ generalised HMC, MEADS warm-up
    def _ghmc_carry(self, C, D, momentum, slice_):
        """The whitened momentum [C, D] and the slice [C] a call works on in place: copies of what was handed in, or
        fresh arrays the kernel fills; and the two has_ flags."""
        f64 = torch.float64
        v = (_dev_f64(momentum, self.device).reshape(C, D).clone() if momentum is not None
             else torch.empty(C, D, dtype=f64, device=self.device))
        u = (_dev_f64(slice_, self.device).reshape(C).clone() if slice_ is not None
             else torch.empty(C, dtype=f64, device=self.device))
        return v, u, int(momentum is not None), int(slice_ is not None)

    def ghmc_sample(self, rng, params, scale, thr, n, q, U, g, momentum=None, slice_=None, keep_samples=True, history=True):
        """``n`` generalised-HMC transitions in one launch (``aehmc_ghmc_sample``).  ``params``: a device tensor [3]
        (eps, alpha, delta) or a tuple of three host floats; ``scale``: a device tensor [1] or [D]."""
        C, D = q.shape
        out, c = self._diag(C, D, False)
        v, u, has_v, has_u = self._ghmc_carry(C, D, momentum, slice_)
        samples, acc, div = self._history_buffers(n, C, D, keep_samples, None) if history else (None, None, None)
        on_device = isinstance(params, torch.Tensor)
        eps, alpha, delta = (0.0, 0.0, 0.0) if on_device else (float(x) for x in params)
        self._check(self.lib.aehmc_ghmc_sample(
            self.ctx, C, rng.data_ptr(), params.data_ptr() if on_device else None, eps, alpha, delta, scale.data_ptr(),
            scale.numel(), float(thr), int(n), q.data_ptr(), U.data_ptr(), g.data_ptr(), v.data_ptr(), has_v,
            u.data_ptr(), has_u, ct.byref(c), samples.data_ptr() if samples is not None else None,
            acc.data_ptr() if history else None, div.data_ptr() if history else None, self.stream), "aehmc_ghmc_sample")
        out["momentum"], out["slice"] = v, u
        out["samples"], out["acceptance_history"], out["divergence_history"] = samples, acc, div
        return out

    def meads_alloc(self, D, initial_step_size, with_sums=False):
        """The state of a MEADS adaptation before any update: params (eps0, 1, 0.5), scale 1 [D], count = skipped = 0;
        ``with_sums``: also ``sums`` [8 + 2 D], which an update fills with its intermediate sums."""
        dev, f64 = self.device, torch.float64
        st = dict(params=torch.tensor([float(initial_step_size), 1.0, 0.5], dtype=f64, device=dev),
                  scale=torch.ones(D, dtype=f64, device=dev),
                  count=torch.zeros(1, dtype=torch.int64, device=dev), skipped=torch.zeros(1, dtype=torch.int64, device=dev))
        if with_sums:
            st["sums"] = torch.zeros(8 + 2 * D, dtype=f64, device=dev)
        return st

    @staticmethod
    def meads_cstate(st):
        return _lib.CMeadsState(**{k: v.data_ptr() for k, v in st.items()})

    def meads_update(self, C, D, position, gradient, multiplier, slowdown, st):
        self._check(self.lib.aehmc_meads_update(self.ctx, C, D, position.data_ptr(), gradient.data_ptr(), float(multiplier),
                                                float(slowdown), ct.byref(self.meads_cstate(st)), self.stream),
                    "aehmc_meads_update")

    def meads_warmup(self, rng, n, multiplier, slowdown, thr, q, U, g, st, momentum=None, slice_=None):
        """The whole MEADS warm-up in one C-ABI call (``aehmc_meads_warmup``): an update, then ``n`` x (transition on
        the state's own parameters, update)."""
        C, D = q.shape
        out, c = self._diag(C, D, False)
        v, u, has_v, has_u = self._ghmc_carry(C, D, momentum, slice_)
        self._check(self.lib.aehmc_meads_warmup(
            self.ctx, C, rng.data_ptr(), int(n), float(multiplier), float(slowdown), float(thr), q.data_ptr(), U.data_ptr(),
            g.data_ptr(), v.data_ptr(), has_v, u.data_ptr(), has_u, ct.byref(c), ct.byref(self.meads_cstate(st)),
            self.stream), "aehmc_meads_warmup")
        out["momentum"], out["slice"] = v, u
        return out

    def syrk_tn(self, X, S, centre=None, w=0.0, delta=None):
        """S[i, j] += sum_c (X[c, i] - centre[i]) (X[c, j] - centre[j]) + w delta[i] delta[j] for j <= i, in place
        (aehmc_syrk_tn; elements above the diagonal are unspecified afterwards)."""
        C, D = X.shape
        self._check(self.lib.aehmc_syrk_tn(self.ctx, C, D, X.data_ptr(), X.stride(0),
                                           centre.data_ptr() if centre is not None else None, float(w),
                                           delta.data_ptr() if delta is not None else None, S.data_ptr(), S.stride(0),
                                           self.stream), "aehmc_syrk_tn")
        return S

    def forget_metric(self):
        """Drop the cache entry of the current shared-metric binding: its arrays were rewritten in place by a kernel
        (which does not move a tensor's version counter), so the key no longer says what they hold."""
        self._metric_cache.pop(self._metric_key, None)
        self._metric_key = None

    def dual_averaging_update(self, target, gamma, t0, kappa, p_accept, step, x, x_avg, g_avg, mu, step_size_out):
        self._check(self.lib.aehmc_dual_averaging_update(
            self.ctx, step.numel(), float(target), float(gamma), float(t0), float(kappa), p_accept.data_ptr(),
            step.data_ptr(), x.data_ptr(), x_avg.data_ptr(), g_avg.data_ptr(), mu.data_ptr(),
            step_size_out.data_ptr() if step_size_out is not None else None, self.stream),
            "aehmc_dual_averaging_update")

    def welford_update(self, value, mean, m2, n, full):
        """algorithms.welford_covariance's update for C estimators, in place (value, mean [C,D]; m2 [C,D] | [C,D,D];
        n [C] int64)."""
        C, D = mean.shape
        self._check(self.lib.aehmc_welford_update(self.ctx, C, D, int(bool(full)), value.data_ptr(), mean.data_ptr(),
                                                  m2.data_ptr(), n.data_ptr(), self.stream), "aehmc_welford_update")

    def covariance_final(self, m2, n, D, full, shrink):
        """m2 / (n - 1) (algorithms.py:199-202), with ``shrink`` Stan's regularisation on top (mass_matrix.py:83-118)."""
        out = torch.empty_like(m2)
        self._check(self.lib.aehmc_covariance_final(self.ctx, n.numel(), int(D), int(bool(full)), int(bool(shrink)),
                                                    m2.data_ptr(), n.data_ptr(), out.data_ptr(), self.stream),
                    "aehmc_covariance_final")
        return out

    # ------------------------------------------------------------------ posterior summaries
    def summary_update(self, chunk, t0, num_draws, n_segments, mean, m2):
        """Fold draws t0 ... t0 + T - 1 (chunk [T, C, D]) into the running moments mean, m2 [n_segments, C, D]."""
        T, C, D = chunk.shape
        self._check(self.lib.aehmc_summary_update(self.ctx, T, C, D, int(t0), int(num_draws), int(n_segments),
                                                  chunk.data_ptr(), mean.data_ptr(), m2.data_ptr(), self.stream),
                    "aehmc_summary_update")

    def summary_autocov(self, samples, n_segments, K, mean):
        """Chain-averaged autocovariance [K, D] of the stored draws [N, C, D] about the split chains' means."""
        N, C, D = samples.shape
        m = n_segments * C
        # groups of split chains: about 1024 workgroups in all, partial sums within 256 MB
        blocks = -(-D // 8)
        G = max(1, min(m, -(-1024 // blocks), (256 << 20) // (8 * K * D), 65535))
        work = torch.empty(G, K, D, dtype=torch.float64, device=self.device)
        acov = torch.empty(K, D, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_summary_autocov(self.ctx, N, C, D, int(n_segments), int(K), G, samples.data_ptr(),
                                                   mean.data_ptr(), work.data_ptr(), acov.data_ptr(), self.stream),
                    "aehmc_summary_autocov")
        return acov

    def summary_lag_group(self, K):
        """Chains per group of the streaming fold at K lags: work is [ceil(C / group), K, D]."""
        return int(self.lib.aehmc_summary_lag_group(int(K)))

    def summary_lag_update(self, chunk, t0, num_draws, n_segments, K, shift, sums, ring, head, work, acov):
        """Fold draws t0 ... t0 + T - 1 (chunk [T, C, D]) into the lagged products work [G, K, D] over the ring of the
        last K - 1 shifted draws; acov [K, D] is complete once the run's last draw has been folded."""
        T, C, D = chunk.shape
        self._check(self.lib.aehmc_summary_lag_update(self.ctx, T, C, D, int(t0), int(num_draws), int(n_segments), int(K),
                                                      chunk.data_ptr(), shift.data_ptr(),
                                                      sums.data_ptr(), ring.data_ptr(), head.data_ptr(), work.data_ptr(),
                                                      acov.data_ptr(), self.stream),
                    "aehmc_summary_lag_update")

    def nested_update(self, chunk, t0, num_draws, window, chains_per_superchain, mean, m2, out):
        """Fold draws t0 ... t0 + T - 1 (chunk [T, C, D]) into the nested R-hat rows out [num_draws / window, 5, D];
        mean, m2 [C, D] carry the chains' moments of the window that stays open."""
        T, C, D = chunk.shape
        self._check(self.lib.aehmc_nested_update(self.ctx, T, C, D, int(t0), int(num_draws), int(window),
                                                 int(chains_per_superchain), chunk.data_ptr(), mean.data_ptr(),
                                                 m2.data_ptr(), out.data_ptr(), self.stream),
                    "aehmc_nested_update")

    def summary_final(self, num_draws, n_segments, mean, m2, acov=None):
        """out [7, D] (mean, sd, rhat, ess, mcse, ess_chains, mcse_chains) and lag_truncated [D] (None without acov)."""
        _, C, D = mean.shape
        out = torch.empty(7, D, dtype=torch.float64, device=self.device)
        trunc = torch.empty(D, dtype=torch.int32, device=self.device) if acov is not None else None
        self._check(self.lib.aehmc_summary_final(self.ctx, int(num_draws), C, D, int(n_segments),
                                                 acov.shape[0] if acov is not None else 0, mean.data_ptr(), m2.data_ptr(),
                                                 acov.data_ptr() if acov is not None else None, out.data_ptr(),
                                                 trunc.data_ptr() if trunc is not None else None, self.stream),
                    "aehmc_summary_final")
        return out, trunc

    def _quantile_work(self, R, D, M):
        nbytes = int(self.lib.aehmc_summary_quantile_work(int(R), int(D), int(M)))
        if nbytes <= 0:
            raise EngineError(f"aehmc_summary_quantile_work: no scratch size for R = {R}, D = {D}, M = {M} (1 <= R < 2^31, "
                              "at most 64 ranks or probabilities a call)")
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def summary_order_stats(self, samples, ranks):
        """out [M, D]: the ranks[i]-th smallest (0-based) value of every coordinate of samples [R, D]."""
        R, D = samples.shape
        M = len(ranks)
        work = self._quantile_work(R, D, M)
        out = torch.empty(M, D, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_summary_order_stats(self.ctx, R, D, M, samples.data_ptr(), (ct.c_int64 * M)(*ranks),
                                                       out.data_ptr(), work.data_ptr(), work.numel(), self.stream),
                    "aehmc_summary_order_stats")
        return out

    def summary_quantiles(self, samples, probs):
        """out [Q, D]: the quantiles (numpy's "linear" rule) of every coordinate of samples [R, D] at probs."""
        R, D = samples.shape
        Q = len(probs)
        work = self._quantile_work(R, D, Q)
        out = torch.empty(Q, D, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_summary_quantiles(self.ctx, R, D, Q, samples.data_ptr(), (ct.c_double * Q)(*probs),
                                                     out.data_ptr(), work.data_ptr(), work.numel(), self.stream),
                    "aehmc_summary_quantiles")
        return out

    def summary_sketch_update(self, chunk, bins, lo, inv_width, counts):
        """Fold chunk [T, C, D] into the histogram counts [D, bins + 3] (int64) on the grid lo, inv_width [D]."""
        T, C, D = chunk.shape
        self._check(self.lib.aehmc_summary_sketch_update(self.ctx, T, C, D, int(bins), chunk.data_ptr(), lo.data_ptr(),
                                                         inv_width.data_ptr(), counts.data_ptr(), self.stream),
                    "aehmc_summary_sketch_update")

    def summary_sketch_quantiles(self, counts, bins, lo, width, probs):
        """(estimate [Q, D], resolved [Q, D] int32) of the histogram counts [D, bins + 3] at probs."""
        D, Q = counts.shape[0], len(probs)
        est = torch.empty(Q, D, dtype=torch.float64, device=self.device)
        res = torch.empty(Q, D, dtype=torch.int32, device=self.device)
        self._check(self.lib.aehmc_summary_sketch_quantiles(self.ctx, D, int(bins), Q, (ct.c_double * Q)(*probs),
                                                            counts.data_ptr(), lo.data_ptr(), width.data_ptr(),
                                                            est.data_ptr(), res.data_ptr(), self.stream),
                    "aehmc_summary_sketch_quantiles")
        return est, res

    def constrain(self, x, table, d_out, out=None):
        """y [R, d_out]: the rows of x [R, D_in] (fp64, contiguous) mapped through ``table``, the per-output entries
        of csrc/constrain.cuh as a uint8 device tensor of 40 * d_out bytes (``transforms.Model`` builds it).  Out of
        place: ``out``, if given, is [R, d_out], fp64, contiguous and shares no memory with x."""
        R, D_in = x.shape
        d_out = int(d_out)
        if x.dtype != torch.float64 or not x.is_contiguous() or x.device != self.device:
            raise ValueError(f"constrain: x must be a contiguous float64 tensor on {self.device}")
        if table.dtype != torch.uint8 or table.numel() != 40 * d_out or table.device != self.device or \
                not table.is_contiguous():
            raise ValueError(f"constrain: the table must hold {d_out} entries of 40 bytes on {self.device}")
        if out is None:
            out = torch.empty(R, d_out, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (R, d_out) or not out.is_contiguous() or \
                out.device != self.device:
            raise ValueError(f"constrain: out must be a contiguous float64 tensor [{R}, {d_out}] on {self.device}")
        if R == 0:
            return out
        lo, hi = x.data_ptr(), x.data_ptr() + 8 * x.numel()
        if out.data_ptr() < hi and lo < out.data_ptr() + 8 * out.numel():
            raise ValueError("constrain: out overlaps the input; the map is out of place")
        self._check(self.lib.aehmc_constrain(self.ctx, R, D_in, d_out, x.data_ptr(), table.data_ptr(), out.data_ptr(),
                                             self.stream),
                    "aehmc_constrain")
        return out

    # ------------------------------------------------------------------ pointwise programs, streaming WAIC
    def set_pointwise(self, owner, traced):
        """Bind the pointwise program ``traced`` (``tracing.TracedPointwise``) of ``owner`` beside the target; a no-op
        while ``owner`` is the one bound.  A source that does not compile raises and leaves the previous program (and the
        arrays it reads) in place; the sampler's target is never touched."""
        if self._keep.get("pointwise", (None,))[0] is owner:
            return
        import os
        arrs = [_dev_f64(a, self.device) for a in traced.params]
        ptrs = (ct.c_void_p * max(len(arrs), 1))(*[a.data_ptr() for a in arrs])
        inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
        src = '#include "dual.cuh"\n' + traced.source
        self._check(self.lib.aehmc_set_pointwise(self.ctx, src.encode(), int(traced.dim), int(traced.n_out),
                                                 int(traced.n_head), ptrs, len(arrs), inc.encode()), "aehmc_set_pointwise")
        self._keep["pointwise"] = (owner, traced, arrs)

    def _rows_f64(self, x, what, width=None):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or not x.is_contiguous() or x.device != self.device \
                or x.ndim != 2 or (width is not None and x.shape[1] != width):
            raise ValueError(f"{what} must be a contiguous float64 tensor [R, {width if width is not None else 'n'}] on "
                             f"{self.device}")

    def pointwise_eval(self, x, out):
        """out [R, n_out] = the bound pointwise program on the rows x [R, D]."""
        _, traced, _ = self._keep["pointwise"]
        self._rows_f64(x, "pointwise_eval: x", traced.dim)
        self._rows_f64(out, "pointwise_eval: out", traced.n_out)
        if out.shape[0] != x.shape[0]:
            raise ValueError("pointwise_eval: x and out differ in their rows")
        if x.shape[0]:
            self._check(self.lib.aehmc_pointwise_eval(self.ctx, x.shape[0], x.data_ptr(), out.data_ptr(), self.stream),
                        "aehmc_pointwise_eval")
        return out

    def pointwise_waic_fold(self, x, state, n_state):
        """Fold the bound program's values of the rows x [R, D] into the WAIC state [4, n_out] behind n_state draws."""
        _, traced, _ = self._keep["pointwise"]
        self._rows_f64(x, "pointwise_waic_fold: x", traced.dim)
        self._rows_f64(state, "pointwise_waic_fold: state", traced.n_out)
        if x.shape[0]:
            self._check(self.lib.aehmc_pointwise_waic_fold(self.ctx, x.shape[0], x.data_ptr(), state.data_ptr(),
                                                           int(n_state), self.stream), "aehmc_pointwise_waic_fold")

    def waic_fold(self, x, state, n_state):
        """Fold the stored block x [R, n_obs] into the WAIC state [4, n_obs] behind n_state draws."""
        self._rows_f64(state, "waic_fold: state")
        self._rows_f64(x, "waic_fold: x", state.shape[1])
        if x.shape[0]:
            self._check(self.lib.aehmc_waic_fold(self.ctx, x.shape[0], x.shape[1], x.data_ptr(), state.data_ptr(),
                                                 int(n_state), self.stream), "aehmc_waic_fold")

    def waic_merge(self, state, n_state, other, n_other):
        self._rows_f64(state, "waic_merge: state")
        self._rows_f64(other, "waic_merge: other", state.shape[1])
        self._check(self.lib.aehmc_waic_merge(self.ctx, state.shape[1], state.data_ptr(), int(n_state), other.data_ptr(),
                                              int(n_other), self.stream), "aehmc_waic_merge")

    def waic_final(self, state, n_state):
        """(lppd [n_obs], p [n_obs]) of the WAIC state behind n_state >= 1 draws."""
        self._rows_f64(state, "waic_final: state")
        lppd, p = (torch.empty(state.shape[1], dtype=torch.float64, device=self.device) for _ in range(2))
        self._check(self.lib.aehmc_waic_final(self.ctx, state.shape[1], state.data_ptr(), int(n_state), lppd.data_ptr(),
                                              p.data_ptr(), self.stream), "aehmc_waic_final")
        return lppd, p

    def summary_rank(self, samples, center, mode, _work_bytes=None):
        """out [R, D]: the average rank (mode 0) or the normal score (mode 1) of every draw of samples [R, D] among the
        draws of its coordinate; with center [D], of the folded draws |samples - center|.  ``_work_bytes``: scratch
        other than the default (the tile of coordinates sorted at a time follows it; the result does not)."""
        R, D = samples.shape
        work = self._rank_work(R, D, _work_bytes)
        out = torch.empty(R, D, dtype=torch.float64, device=self.device)
        self._check(self.lib.aehmc_summary_rank(self.ctx, R, D, samples.data_ptr(),
                                                center.data_ptr() if center is not None else None, int(mode),
                                                out.data_ptr(), work.data_ptr(), work.numel(), self.stream),
                    "aehmc_summary_rank")
        return out

    def _rank_work(self, R, D, _work_bytes):
        """The scratch of the calls that sort: the default size, or ``_work_bytes``."""
        nbytes = int(self.lib.aehmc_summary_rank_work(int(R), int(D))) if _work_bytes is None else int(_work_bytes)
        if nbytes <= 0:
            raise EngineError(f"aehmc_summary_rank_work: no scratch size for R = {R}, D = {D} (1 <= R < 2^31)")
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def summary_hdi(self, samples, prob, _work_bytes=None):
        """(lower [D], upper [D], index [D] int64): the narrowest window of min(floor(prob R), R - 1) + 1 consecutive
        order statistics of every coordinate of samples [R, D], and where it starts.  ``_work_bytes`` as in
        ``summary_rank``."""
        R, D = samples.shape
        work = self._rank_work(R, D, _work_bytes)
        lower, upper = (torch.empty(D, dtype=torch.float64, device=self.device) for _ in range(2))
        index = torch.empty(D, dtype=torch.int64, device=self.device)
        self._check(self.lib.aehmc_summary_hdi(self.ctx, R, D, samples.data_ptr(), float(prob), lower.data_ptr(),
                                               upper.data_ptr(), index.data_ptr(), work.data_ptr(), work.numel(),
                                               self.stream),
                    "aehmc_summary_hdi")
        return lower, upper, index

    def summary_quantile_mcse(self, samples, probs, ess, _work_bytes=None):
        """(out [Q, D], ranks [2, Q, D] int64): the MCSE of the quantiles of samples [R, D] at probs, from the
        effective sample sizes ess [Q, D] (device) of the indicators, and the two order statistics behind each."""
        R, D = samples.shape
        Q = len(probs)
        work = self._rank_work(R, D, _work_bytes)
        out = torch.empty(Q, D, dtype=torch.float64, device=self.device)
        ranks = torch.empty(2, Q, D, dtype=torch.int64, device=self.device)
        self._check(self.lib.aehmc_summary_quantile_mcse(self.ctx, R, D, Q, samples.data_ptr(),
                                                         (ct.c_double * Q)(*probs), ess.data_ptr(), out.data_ptr(),
                                                         ranks.data_ptr(), work.data_ptr(), work.numel(), self.stream),
                    "aehmc_summary_quantile_mcse")
        return out, ranks

    def beta_quantile(self, p, a, b):
        """out shaped like p: the x with I_x(a, b) = p, elementwise over float64 device tensors of one shape."""
        out = torch.empty_like(p)
        self._check(self.lib.aehmc_beta_quantile(self.ctx, p.numel(), p.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                 out.data_ptr(), self.stream),
                    "aehmc_beta_quantile")
        return out

    def summary_psis(self, log_ratios, reff=None, log_values=None, weights=True, _work_bytes=None):
        """(log_weights [R, D] or None, pareto_k [D], tail_len [D] int64, log_mean [D] or None): Pareto-smoothed
        importance sampling of every column of log_ratios [R, D]; reff [D] (device) or None for 1.  With log_values
        [R, D], log_mean = log sum exp(log_weights + log_values); ``log_ratios=None`` then means -log_values (PSIS-LOO
        of a log-likelihood, without a negated copy).  ``weights=False``: the log-weights are not stored.
        ``_work_bytes`` as in ``summary_rank``."""
        R, D = (log_ratios if log_ratios is not None else log_values).shape
        work = self._rank_work(R, D, _work_bytes)
        lw = torch.empty(R, D, dtype=torch.float64, device=self.device) if weights else None
        k = torch.empty(D, dtype=torch.float64, device=self.device)
        tail = torch.empty(D, dtype=torch.int64, device=self.device)
        mean = torch.empty(D, dtype=torch.float64, device=self.device) if log_values is not None else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._check(self.lib.aehmc_summary_psis(self.ctx, R, D, ptr(log_ratios), ptr(reff), ptr(log_values), ptr(lw),
                                                k.data_ptr(), tail.data_ptr(), ptr(mean), work.data_ptr(), work.numel(),
                                                self.stream),
                    "aehmc_summary_psis")
        return lw, k, tail, mean

    def profile_enable(self, on=True):
        self._check(self.lib.aehmc_profile_enable(self.ctx, int(on)), "aehmc_profile_enable")

    def profile_read(self):
        ms, n, fl = ct.c_double(), ct.c_int64(), ct.c_double()
        self._check(self.lib.aehmc_profile_read(self.ctx, ct.byref(ms), ct.byref(n), ct.byref(fl)),
                    "aehmc_profile_read")
        return ms.value, n.value, fl.value


_engines = {}


def get_engine(device=None) -> Engine:
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}") \
        if torch.cuda.is_available() else None
    if dev is None:
        return Engine(device)  # raises the loud error
    if dev not in _engines:
        _engines[dev] = Engine(dev)
    return _engines[dev]


def rng_to_device(sites: np.ndarray, device) -> torch.Tensor:
    """uint64 [C,n,4] -> int64 device tensor with the same bits."""
    return torch.from_numpy(np.ascontiguousarray(sites).view(np.int64)).to(device)
