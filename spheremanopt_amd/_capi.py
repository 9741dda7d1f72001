"""ctypes binding of libsmo.so (C-ABI: include/smo.h).

There is no CPU fallback: if the library is missing or no HIP device is usable the calls raise.
Build the library with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C spheremanopt_amd/csrc``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMO_LIB", os.path.join(_HERE, "lib", "libsmo.so"))      # SMO_LIB: experimental builds

# ---- the header's values, mirrored once (tests/test_capi.py compares every one of them with include/smo.h) -------------------------
SMO_SH23, SMO_SHB23, SMO_KDYN, SMO_POIS = 1, 2, 3, 4                               # smo_config.kind
COST = {"Final": 0, "Integrated": 1}                                              # SMO_COST_*
ADJOINT = {"Discrete": 0, "Continuous": 1}                                        # SMO_ADJ_*
ERR_NAMES = {1: "SMO_ERR_ARG", 2: "SMO_ERR_NO_DEVICE", 3: "SMO_ERR_HIP", 4: "SMO_ERR_STATE", 5: "SMO_ERR_NOMEM",
             6: "SMO_ERR_UNSUPPORTED"}
# `op` of smo_kdyn_op: the phases between two exchanges of the slab-decomposed time loop (kdyn_slab.py)
SMO_KD_SET_BUFFERS, SMO_KD_EXCHANGE_ELEMS, SMO_KD_G2C_A, SMO_KD_G2C_C, SMO_KD_C2G_A, SMO_KD_C2G_B = 0, 1, 2, 3, 4, 5
SMO_KD_FWD_A, SMO_KD_FWD_B, SMO_KD_FWD_C, SMO_KD_ENERGY = 6, 7, 8, 9
SMO_KD_ADJ_INIT, SMO_KD_ADJ_A, SMO_KD_ADJ_B, SMO_KD_ADJ_C = 10, 11, 12, 13
SMO_KD_SYNC, SMO_KD_SET_CHUNKS, SMO_KD_NU_B, SMO_KD_NU_C = 14, 15, 16, 17


class smo_config(C.Structure):
    _fields_ = [("kind", C.c_int), ("npts", C.c_int), ("x0", C.c_double), ("x1", C.c_double), ("dt", C.c_double),
                ("n_iters", C.c_int), ("param", C.c_double), ("cost", C.c_int), ("batch", C.c_int), ("device", C.c_int),
                ("rank", C.c_int), ("world", C.c_int), ("ckpt", C.c_int),
                ("npts2", C.c_int), ("param2", C.c_double), ("param3", C.c_double), ("param4", C.c_double)]


ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)      # smo_alltoall_fn
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)                       # smo_allreduce_fn

# ---- every exported function: name -> (restype, argtypes) ------------------------------------------------------------------------
_int, _dbl, _vp, _sz, _str = C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_char_p
_ip, _dp, _pp, _szp = C.POINTER(_int), C.POINTER(_dbl), C.POINTER(_vp), C.POINTER(_sz)
SIGNATURES = {
    "smo_create": (_int, [C.POINTER(smo_config), _pp]),
    "smo_create_multi": (_int, [C.POINTER(smo_config), _int, _ip, _pp]),
    "smo_create_members": (_int, [C.POINTER(smo_config), _dp, _pp]),
    "smo_create_frozen_u": (_int, [C.POINTER(smo_config), _dp, _int, _pp]),
    "smo_set_horizons": (_int, [_vp, _ip]),
    "smo_get_horizons": (_int, [_vp, _ip]),
    "smo_destroy": (None, [_vp]),
    "smo_last_error": (_str, []),
    "smo_version": (_str, []),
    "smo_device_count": (_int, [_ip]),
    "smo_device_cus": (_int, [_int, _ip]),
    "smo_ncomp": (_int, [_vp]),
    "smo_vec_len": (_int, [_vp, _szp]),
    "smo_stack_bytes": (_int, [_vp, _szp]),
    "smo_get": (_int, [_vp, _int, _dp]),
    "smo_forward": (_int, [_vp, _pp, _dp]),
    "smo_adjoint": (_int, [_vp, _pp, _int, _pp]),
    "smo_inner": (_int, [_vp, _vp, _vp, _dp]),
    "smo_forward_dev": (_int, [_vp, _pp, _dp]),
    "smo_adjoint_dev": (_int, [_vp, _pp, _int, _pp]),
    "smo_inner_dev": (_int, [_vp, _vp, _vp, _dp]),
    "smo_inner_slabs": (_int, [_vp, _pp, _pp, _dp]),
    "smo_hessvec": (_int, [_vp, _pp, _pp, _dp]),
    "smo_hessvec_dev": (_int, [_vp, _pp, _pp, _dp]),
    "smo_gram": (_int, [_vp, _vp, _vp, _dp]),
    "smo_gram_dev": (_int, [_vp, _vp, _vp, _dp]),
    "smo_combine": (_int, [_vp, _dp, _vp, _vp]),
    "smo_combine_dev": (_int, [_vp, _dp, _vp, _vp]),
    "smo_gram_geometry": (_int, [_vp, _szp]),
    "smo_snapshot_len": (_int, [_vp, _szp]),
    "smo_snapshot_read": (_int, [_vp, _int, _int, _dp]),
    "smo_transform": (_int, [_vp, _int, _vp, _vp]),
    "smo_kdyn_op": (_int, [_vp, _int, _int, _int, _vp, _vp, _dp]),
    "smo_set_stream": (_int, [_vp, _vp]),
    "smo_timing_enable": (_int, [_vp, _int]),
    "smo_timing_select": (_int, [_vp, C.c_ulonglong]),
    "smo_timing_stride": (_int, [_vp, _int]),
    "smo_timing_classes": (_int, [_vp]),
    "smo_timing_get": (_int, [_vp, _int, C.POINTER(_str), C.POINTER(C.c_longlong), _dp, _dp]),
    "smo_timing_hbm_bytes": (_int, [_vp, _int, _dp]),
    "smo_vec_alloc": (_int, [_int, _sz, _pp]),
    "smo_vec_free": (_int, [_int, _vp]),
    "smo_vec_pool_release": (_int, [_int]),
    "smo_vec_pool_bytes": (_int, [_int, _szp, _szp]),
    "smo_vec_upload": (_int, [_int, _vp, _vp, _sz]),
    "smo_vec_download": (_int, [_int, _vp, _vp, _sz]),
    "smo_vec_axpby": (_int, [_int, _sz, _dbl, _vp, _dbl, _vp, _vp]),
    "smo_host_alloc": (_int, [_sz, _pp]),
    "smo_host_free": (_int, [_vp]),
    "smo_guard_report": (_int, [_vp, _szp, _szp, _vp, _sz]),
    "smo_lds_probe": (_int, [_int, _sz, _sz, _szp, _szp, _szp, _szp]),
    "smo_comm_unique_id": (_int, [_vp]),
    "smo_comm_init": (_int, [_vp, _vp]),
    "smo_comm_set_transport": (_int, [_vp, ALLTOALL_FN, ALLREDUCE_FN, _vp]),
    "smo_comm_get": (_int, [_vp, _int, _dp]),
    "smo_comm_library": (_str, []),
}
EXPORTS = list(SIGNATURES)


class SmoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, "error %d" % code), msg))
        self.code = code


_lib = None


def _preload_torch_lib(filename):
    """PyTorch-ROCm wheels bundle their own libamdhip64.so and librccl.so.  Two HIP runtimes in one process do not work (the second one
    finds no GPU), so if torch is installed its runtime is loaded first and libsmo's DT_NEEDED libamdhip64 resolves to it; this keeps
    `import torch` (bench.py, the multi-GPU driver) usable in either import order.  Likewise libsmo must use the librccl that is going to
    live in this process (smo_comm_init picks up an already loaded librccl.so.1 before looking for the system one).  torch itself is
    not imported."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", filename)
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libsmo.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libsmo.so not found at %s — the HIP extension is not built (run __graft_entry__.build()); "
                           "spheremanopt_amd has no CPU fallback" % LIB_PATH)
    _preload_torch_lib("libamdhip64.so")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise SmoError(rc, lib().smo_last_error().decode())


def comm_unique_id():
    """128 opaque bytes (an RCCL unique id) made by ONE rank and handed to every rank's Context.comm_init."""
    _preload_torch_lib("librccl.so")
    buf = C.create_string_buffer(128)
    _check(lib().smo_comm_unique_id(buf))
    return buf.raw


def device_count():
    n = C.c_int(0)
    lib().smo_device_count(C.byref(n))
    return n.value


def device_cus(device=0):
    """Compute units of a device."""
    n = C.c_int(0)
    _check(lib().smo_device_cus(device, C.byref(n)))
    return n.value


def guard_report(ctx=None):
    """smo_guard_report -> (blocks checked, blocks damaged, description of the first damage or ""): the guard zones of SMO_GUARD around the
    live blocks of `ctx` (a Context, or None), around every device vector, and what the frees recorded since the last report."""
    checked, damaged, first = C.c_size_t(), C.c_size_t(), C.create_string_buffer(512)
    _check(lib().smo_guard_report(ctx._h if ctx is not None else None, C.byref(checked), C.byref(damaged), first, len(first)))
    return checked.value, damaged.value, first.value.decode()


def lds_probe(lds_bytes=0, workgroups=0, device=0):
    """smo_lds_probe (test infrastructure, SMO_POISON_LDS) -> (words probed, words that equal the fill word, fill dispatches, launches that
    found the knob set): `workgroups` workgroups each read their `lds_bytes` of LDS without writing them; the two counters are process-wide
    since the last call and are reset.  Without arguments nothing is launched: the knob is read and the counters are taken."""
    out = [C.c_size_t() for _ in range(4)]
    _check(lib().smo_lds_probe(device, lds_bytes, workgroups, *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def _ptr_array(ptrs):
    arr = (C.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def _dev_ptr(t):
    """Device address of a DeviceVector (.ptr), a torch tensor (.data_ptr()) or a plain int."""
    if isinstance(t, int):
        return t
    p = getattr(t, "ptr", None)
    return int(p) if p is not None else int(t.data_ptr())


def _describe_vec(v, who):
    """(entries, device ordinal) of a device vector that describes itself — a DeviceVector (.n, .device) or a torch tensor (numel(),
    .device) — with None for what it does not tell.  A tensor that is not contiguous float64 is refused here."""
    n = getattr(v, "n", None)
    if n is None and hasattr(v, "numel"):
        n = v.numel()
        if getattr(v, "dtype", None) is not None and getattr(v.dtype, "itemsize", 8) != 8:
            raise ValueError("%s: float64 vectors expected, got %s" % (who, v.dtype))
        if hasattr(v, "is_contiguous") and not v.is_contiguous():
            raise ValueError("%s: contiguous vectors expected" % who)
    dev = getattr(v, "device", None)
    idx = dev if isinstance(dev, int) else getattr(dev, "index", None)
    return (None if n is None else int(n)), (None if idx is None else int(idx))


def check_horizons(n_iters):
    """A sequence of step counts, one per member -> tuple of ints; ValueError for an empty one, a non-integer or a value < 1 (no device call)."""
    try:
        vals = list(n_iters)
    except TypeError:
        raise ValueError("horizons: a sequence of step counts expected, got %r" % (n_iters,)) from None
    if not vals:
        raise ValueError("horizons: an empty sequence (one number of steps per member expected)")
    out = []
    for b, v in enumerate(vals):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("horizon of member %d is %r: an integer number of steps expected" % (b, v))
        if v < 1:
            raise ValueError("horizon of member %d is %d: at least one step" % (b, v))
        out.append(int(v))
    return tuple(out)


def _per_member(values):
    """One value per batch member as the callbacks return them: a float for a batch-1 context, else the array."""
    return float(values[0]) if values.size == 1 else values


class _PinnedBlock:
    """Owner of one hipHostMalloc block; the NumPy arrays made from it keep it alive through their .base chain."""

    def __init__(self, nbytes):
        self.p = C.c_void_p()
        _check(lib().smo_host_alloc(int(nbytes), C.byref(self.p)))
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.p.value:
                lib().smo_host_free(self.p)
                self.p = C.c_void_p()
        except Exception:
            pass


def pinned_empty(n):
    """float64[n] in page-locked host memory (smo_host_alloc): the host-buffer entry points then copy at PCIe rate."""
    blk = _PinnedBlock(8 * int(n))
    raw = (C.c_double * int(n)).from_address(blk.p.value)
    raw._smo_block = blk                       # the ctypes array is the ndarray's base and carries the block
    return np.frombuffer(raw, dtype=np.float64, count=int(n))


def pinned_copy(x):
    out = pinned_empty(np.asarray(x).size)
    out[:] = np.asarray(x, dtype=np.float64).reshape(-1)
    return out


class Context:
    """Owner of one smo_ctx (device buffers, twiddles, the HBM snapshot stack)."""
    devices = None          # MultiContext: the device list
    params = None           # a context made with one `param` per member (smo_create_members): the values, a tuple of floats
    frozen_u = False        # a KDYN context with a frozen velocity (smo_create_frozen_u): adjoint* return [dJ/dB0] alone
    keep_states = True

    def __init__(self, kind, npts, interval, dt, n_iters, param, cost="Final", batch=1, device=0, rank=0, world=1, ckpt=1,
                 npts2=0, param2=0., param3=0., param4=0., frozen_u=False, keep_states=True):
        """`param` a sequence (KDYN: Rm, SH23: a): one value per member, smo_create_members with batch = len(param); an explicit `batch`
        must then be 1 or that length.
        frozen_u (KDYN, one GPU): smo_create_frozen_u — the velocity is given, the adjoint computes dJ/dB0 alone; keep_states=False
        (Final cost only) then keeps no snapshot stack either."""
        members = None
        if np.ndim(param) != 0:
            members = tuple(float(p) for p in np.asarray(param, dtype=np.float64).reshape(-1))
            if int(batch) not in (1, len(members)):
                raise ValueError("batch = %d contradicts the %d values of param (one per member)" % (batch, len(members)))
            batch, param = len(members), (members[0] if members else 0.)
        cfg = smo_config(kind, int(npts), float(interval[0]), float(interval[1]), float(dt), int(n_iters), float(param),
                         COST[cost] if isinstance(cost, str) else int(cost), int(batch), int(device), int(rank), int(world),
                         int(ckpt), int(npts2), float(param2), float(param3), float(param4))
        if frozen_u:
            values = None if members is None else (C.c_double * len(members))(*members)
            self.frozen_u, self.keep_states = True, bool(keep_states)
            self._create(cfg, lambda c, h: lib().smo_create_frozen_u(c, values, 1 if keep_states else 0, h))
            self.params = members
        elif not keep_states:
            raise ValueError("keep_states=False needs frozen_u=True (the full adjoint reads every forward state)")
        elif members is None:
            self._create(cfg, lambda c, h: lib().smo_create(c, h))
        else:
            values = (C.c_double * len(members))(*members)
            self._create(cfg, lambda c, h: lib().smo_create_members(c, values, h))
            self.params = members

    def _create(self, cfg, call):
        """Open the handle with `call(config pointer, handle pointer)` and read the context's geometry back."""
        self.cfg, self.batch, self._h = cfg, cfg.batch, C.c_void_p()
        _check(call(C.byref(cfg), C.byref(self._h)))
        self.ncomp = lib().smo_ncomp(self._h)
        self.ngrad = 1 if self.frozen_u else self.ncomp          # gradient vectors the adjoint fills
        n = C.c_size_t()
        _check(lib().smo_vec_len(self._h, C.byref(n)))
        self.vec_len = n.value
        _check(lib().smo_stack_bytes(self._h, C.byref(n)))
        self.stack_bytes = n.value
        _check(lib().smo_snapshot_len(self._h, C.byref(n)))
        self.snapshot_len = n.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().smo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- a time horizon of its own for every member (smo_set_horizons; KDYN on one GPU, SH23) ---------------------------------------------
    _horizons = None

    def set_horizons(self, n_iters):
        """One number of steps per member, each in [1, the n_iters the context was created with]; None: every member back to that.  The
        next call must be a forward solve; snapshot(i, b) then counts member b's own time."""
        if n_iters is None:
            _check(lib().smo_set_horizons(self._h, None))
            self._horizons = None
            return
        hz = tuple(int(v) for v in n_iters)                  # (the range is the library's to check: its message names the member)
        if len(hz) != self.batch:
            raise ValueError("set_horizons: %d values for the %d members of the context" % (len(hz), self.batch))
        _check(lib().smo_set_horizons(self._h, (C.c_int * len(hz))(*hz)))
        self._horizons = hz

    @property
    def horizons(self):
        """The members' horizons (a tuple of ints) or None when none are set."""
        return self._horizons

    # -- host-buffer entry points --------------------------------------------------------------------------------
    def _host_vecs(self, X):
        vs = [np.ascontiguousarray(np.asarray(X[c], dtype=np.float64)).reshape(-1) for c in range(self.ncomp)]
        for v in vs:
            if v.size != self.vec_len * self.batch:
                raise ValueError("vector has %d entries, context expects %d" % (v.size, self.vec_len * self.batch))
        return vs

    def forward(self, X):
        vs = self._host_vecs(X)
        J = np.zeros(self.batch)
        _check(lib().smo_forward(self._h, _ptr_array([v.ctypes.data for v in vs]), J.ctypes.data_as(C.POINTER(C.c_double))))
        return _per_member(J)

    def adjoint(self, X=None, adjoint_type="Discrete", out=None):
        """`out`: caller-owned result arrays (e.g. pinned ones), else fresh NumPy arrays like the reference's."""
        grads = out if out is not None else [np.empty(self.vec_len * self.batch) for _ in range(self.ngrad)]
        if len(grads) != self.ngrad:
            raise ValueError("adjoint(out=): %d arrays given, the context fills %d" % (len(grads), self.ngrad))
        for g in grads:
            if g.size != self.vec_len * self.batch or g.dtype != np.float64 or not g.flags.c_contiguous:
                raise ValueError("adjoint(out=): contiguous float64 arrays of %d entries expected" % (self.vec_len * self.batch))
        if X is None:
            xp = _ptr_array([None] * self.ncomp)
        else:
            vs = self._host_vecs(X)
            xp = _ptr_array([v.ctypes.data for v in vs])
        gp = _ptr_array([g.ctypes.data for g in grads] + [None] * (self.ncomp - self.ngrad))
        _check(lib().smo_adjoint(self._h, xp, ADJOINT[adjoint_type], gp))
        return grads

    def inner(self, x, y):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if x.size != self.vec_len * self.batch or y.size != x.size:
            raise ValueError("inner: vectors have %d/%d entries, context expects %d" % (x.size, y.size, self.vec_len * self.batch))
        out = np.zeros(self.batch)
        _check(lib().smo_inner(self._h, x.ctypes.data, y.ctypes.data, out.ctypes.data_as(C.POINTER(C.c_double))))
        return _per_member(out)

    # -- device-resident entry points (torch tensors on the context's device, or raw addresses) ------------------------
    _ANY_COUNT = ("inner", "gram_dev", "combine_dev", "hessvec_dev")     # callers that hand over their own number of single-component vectors

    def _check_dev(self, vecs, who):
        """A device vector of the wrong length or on another GPU would be an out-of-bounds device access, not an exception: refuse it
        here.  (Raw integer addresses cannot be checked — the caller vouches for them, as across the C-ABI itself.)"""
        want_n = self.ngrad if who == "adjoint_dev(grads)" else self.ncomp
        if len(vecs) != want_n and who not in self._ANY_COUNT:
            raise ValueError("%s: %d vectors given, the context expects %d" % (who, len(vecs), want_n))
        want = self.vec_len * self.batch
        for v in vecs:
            if isinstance(v, int):
                continue
            n, idx = _describe_vec(v, who)
            if n is not None and n != want:
                raise ValueError("%s: device vector has %d entries, context expects %d" % (who, n, want))
            if getattr(getattr(v, "device", None), "type", "cuda") != "cuda":
                raise ValueError("%s: vector lives on %s, not on a GPU" % (who, v.device))
            if idx is not None and idx != self.cfg.device:
                raise ValueError("%s: vector lives on device %d, the context on device %d" % (who, idx, self.cfg.device))

    def forward_dev(self, X):
        self._check_dev(X, "forward_dev")
        J = np.zeros(self.batch)
        _check(lib().smo_forward_dev(self._h, _ptr_array([_dev_ptr(x) for x in X]), J.ctypes.data_as(C.POINTER(C.c_double))))
        return _per_member(J)

    def adjoint_dev(self, X, grads, adjoint_type="Discrete"):
        if X is not None:
            self._check_dev(X, "adjoint_dev")
        self._check_dev(grads, "adjoint_dev(grads)")
        xp = _ptr_array([_dev_ptr(x) for x in X]) if X is not None else _ptr_array([None] * self.ncomp)     # the adjoint replays the stack: X is not read
        gp = _ptr_array([_dev_ptr(g) for g in grads] + [None] * (self.ncomp - self.ngrad))
        _check(lib().smo_adjoint_dev(self._h, xp, ADJOINT[adjoint_type], gp))
        return grads

    def inner_dev(self, x, y):
        self._check_dev([x, y], "inner")
        out = np.zeros(self.batch)
        _check(lib().smo_inner_dev(self._h, _dev_ptr(x), _dev_ptr(y), out.ctypes.data_as(C.POINTER(C.c_double))))
        return _per_member(out)

    # -- either kind of vector: NumPy arrays (staged over PCIe) or devvec.DeviceVector (already in HBM) ---------------------------------
    @staticmethod
    def _on_device(v):
        return hasattr(v, "ptr") and hasattr(v, "numpy")

    def forward_any(self, X):
        return self.forward_dev(X) if self._on_device(X[0]) else self.forward(X)

    def adjoint_any(self, X, adjoint_type="Discrete"):
        """Device vectors in -> fresh device vectors out (like the reference's fresh arrays); anything else: NumPy arrays out."""
        if X is not None and len(X) and self._on_device(X[0]):
            from .devvec import DeviceVector
            grads = [DeviceVector(self.vec_len * self.batch, self.cfg.device) for _ in range(self.ngrad)]
            self.adjoint_dev(list(X), grads, adjoint_type)
            return grads
        return self.adjoint(None, adjoint_type)

    def inner_any(self, x, y):
        dx, dy = self._on_device(x), self._on_device(y)
        if dx and dy:
            return self.inner_dev(x, y)
        if dx or dy:
            raise TypeError("inner product: one operand is a DeviceVector and the other is not")
        return self.inner(x, y)

    # -- Hessian-vector products of the discrete cost (smo_hessvec*; SH23): valid after a forward solve, any number of directions ---------
    def _hessvec_done(self, dJ):
        n = C.c_size_t()
        _check(lib().smo_stack_bytes(self._h, C.byref(n)))       # the tangent stack exists from the first product on
        self.stack_bytes = n.value
        return _per_member(dJ)

    def hessvec(self, V, out=None):
        """(HV, dJ): HV = [H.V] as adjoint returns the gradient ([batch*G]; `out`: a caller-owned list of one such array), dJ = <V, grad f>
        per member as the tangent sweep accumulates it (a float for batch 1)."""
        v = np.ascontiguousarray(np.asarray(V[0] if isinstance(V, (list, tuple)) else V, dtype=np.float64)).reshape(-1)
        n = self.vec_len * self.batch
        if v.size != n:
            raise ValueError("hessvec: direction has %d entries, context expects %d" % (v.size, n))
        HV = out if out is not None else [np.empty(n)]
        if len(HV) != 1 or HV[0].size != n or HV[0].dtype != np.float64 or not HV[0].flags.c_contiguous:
            raise ValueError("hessvec(out=): a list of one contiguous float64 array of %d entries expected" % n)
        dJ = np.zeros(self.batch)
        _check(lib().smo_hessvec(self._h, _ptr_array([v.ctypes.data]), _ptr_array([HV[0].ctypes.data]), dJ.ctypes.data_as(_dp)))
        return HV, self._hessvec_done(dJ)

    def hessvec_dev(self, V, HV):
        """The same on device vectors: V, HV lists of one device vector each (HV is filled); returns (HV, dJ)."""
        self._check_dev(list(V) + list(HV), "hessvec_dev")
        if len(V) != 1 or len(HV) != 1:
            raise ValueError("hessvec_dev: V and HV are lists of one device vector each")
        dJ = np.zeros(self.batch)
        _check(lib().smo_hessvec_dev(self._h, _ptr_array([_dev_ptr(V[0])]), _ptr_array([_dev_ptr(HV[0])]), dJ.ctypes.data_as(_dp)))
        return HV, self._hessvec_done(dJ)

    def hessvec_any(self, V):
        """Device vectors in -> a fresh device vector out; anything else: NumPy arrays.  Returns (HV, dJ)."""
        if len(V) and self._on_device(V[0]):
            from .devvec import DeviceVector
            return self.hessvec_dev(list(V), [DeviceVector(self.vec_len * self.batch, self.cfg.device)])
        return self.hessvec(V)

    # -- across the members: Gram matrix <x_a, y_b> and recombination out_b = sum_a C[a][b] x_a (smo_gram*, smo_combine*) ---------------
    def _block_refuse_multi(self, who):
        if self.devices is not None:
            raise ValueError("%s: not available on a multi-device context (its vectors are distributed over the devices)" % who)

    def _block_coeffs(self, Cm, who):
        Cm = np.ascontiguousarray(Cm, dtype=np.float64)
        if Cm.shape != (self.batch, self.batch):
            raise ValueError("%s: C has shape %s, the context's %d members need (%d, %d)" % (who, Cm.shape, self.batch, self.batch, self.batch))
        return Cm

    def _block_host(self, v, who):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if v.size != self.vec_len * self.batch:
            raise ValueError("%s: vector has %d entries, context expects %d" % (who, v.size, self.vec_len * self.batch))
        return v

    def gram(self, x, y=None):
        """(B, B) array of <x_a, y_b> in the context's inner product, host vectors [B][vec_len]; y=None: the exactly symmetric <x_a, x_b>."""
        self._block_refuse_multi("gram")
        x = self._block_host(x, "gram")
        y = x if y is None else self._block_host(y, "gram")
        out = np.zeros((self.batch, self.batch))
        _check(lib().smo_gram(self._h, x.ctypes.data, y.ctypes.data, out.ctypes.data_as(_dp)))
        return out

    def gram_dev(self, x, y=None):
        self._block_refuse_multi("gram_dev")
        y = x if y is None else y
        self._check_dev([x, y], "gram_dev")
        out = np.zeros((self.batch, self.batch))
        _check(lib().smo_gram_dev(self._h, _dev_ptr(x), _dev_ptr(y), out.ctypes.data_as(_dp)))
        return out

    def combine(self, Cm, x):
        """out_b = sum_a C[a][b] x_a on host vectors [B][vec_len] (X.C with the members as columns); returns a fresh array."""
        self._block_refuse_multi("combine")
        Cm = self._block_coeffs(Cm, "combine")
        x = self._block_host(x, "combine")
        out = np.empty_like(x)
        _check(lib().smo_combine(self._h, Cm.ctypes.data_as(_dp), x.ctypes.data, out.ctypes.data))
        return out

    def combine_dev(self, Cm, x, out=None):
        """The same on a device vector; `out`: a DeviceVector to fill (not x itself), else a fresh one.  Returns it."""
        self._block_refuse_multi("combine_dev")
        Cm = self._block_coeffs(Cm, "combine_dev")
        if out is x:
            raise ValueError("combine_dev: out is x (every output member reads every input member: the product is not done in place)")
        self._check_dev([x] if out is None else [x, out], "combine_dev")
        if out is None:
            from .devvec import DeviceVector
            out = DeviceVector(self.vec_len * self.batch, self.cfg.device)
        _check(lib().smo_combine_dev(self._h, Cm.ctypes.data_as(_dp), _dev_ptr(x), _dev_ptr(out)))
        return out

    def gram_geometry(self):
        """How gram* cuts the element axis here: {"chunk": elements per chunk, "chunks_per_workgroup", "workgroups", "combine_workgroup"}."""
        geo = (C.c_size_t * 4)()
        _check(lib().smo_gram_geometry(self._h, geo))
        return dict(zip(("chunk", "chunks_per_workgroup", "workgroups", "combine_workgroup"), (int(v) for v in geo)))

    def gram_any(self, x, y=None):
        dx, dy = self._on_device(x), (self._on_device(x) if y is None else self._on_device(y))
        if dx and dy:
            return self.gram_dev(x, y)
        if dx or dy:
            raise TypeError("Gram matrix: one operand is a DeviceVector and the other is not")
        return self.gram(x, y)

    def combine_any(self, Cm, x):
        return self.combine_dev(Cm, x) if self._on_device(x) else self.combine(Cm, x)

    # -- slab communicator (KDYN, world > 1): the transposes then happen inside smo_forward / smo_adjoint ----------------
    def comm_init(self, unique_id):
        """Collective: RCCL communicator over the context's `world` ranks from the 128 bytes of comm_unique_id()."""
        _preload_torch_lib("librccl.so")
        if len(unique_id) != 128:
            raise ValueError("comm_init: the unique id has 128 bytes")
        _check(lib().smo_comm_init(self._h, C.create_string_buffer(bytes(unique_id), 128)))

    def comm_set_transport(self, all_to_all, all_reduce_sum):
        """Collective: caller-provided transport instead of RCCL.  all_to_all(src_dev, dst_dev, bytes_per_peer, hip_stream) and
        all_reduce_sum(ctypes double pointer, n) are Python callables (exceptions are reported as a failed exchange)."""
        def a2a(user, src, dst, nbytes, stream):
            try:
                all_to_all(src, dst, nbytes, stream)
                return 0
            except Exception as e:               # noqa: BLE001 — an exception must not unwind through the C frames
                self._transport_error = e
                return 1

        def ared(user, vals, n):
            try:
                all_reduce_sum(vals, n)
                return 0
            except Exception as e:               # noqa: BLE001
                self._transport_error = e
                return 1

        self._transport = (ALLTOALL_FN(a2a), ALLREDUCE_FN(ared))          # keep the thunks alive as long as the context
        self._transport_error = None
        _check(lib().smo_comm_set_transport(self._h, self._transport[0], self._transport[1], None))

    def comm_get(self, key):
        v = C.c_double()
        _check(lib().smo_comm_get(self._h, int(key), C.byref(v)))
        return v.value

    # -- introspection ------------------------------------------------------------------------------------------------
    def snapshot(self, index, b=0):
        out = np.empty(self.snapshot_len)
        _check(lib().smo_snapshot_read(self._h, int(b), int(index), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def transform(self, which, x, out_len=None):
        """smo_transform; `out_len` = doubles of the result when it differs from the input (POIS: grid <-> complex coefficients)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x) if out_len is None else np.empty(int(out_len))
        _check(lib().smo_transform(self._h, int(which), x.ctypes.data, out.ctypes.data))
        return out

    def get(self, key):
        v = C.c_double()
        _check(lib().smo_get(self._h, int(key), C.byref(v)))
        return v.value

    def timing_enable(self, on=True, only=None, select=None, every=1):
        """on=False: off; on=True: every kernel class; only=k: just class k (index into timing()); select=[k, ...]: exactly those classes;
        every=n: of those, every n-th launch only (a uniform sample at 1/n of the event overhead)."""
        _check(lib().smo_timing_stride(self._h, int(every)))
        if select is not None:
            mask = 0
            for k in select:
                mask |= 1 << int(k)
            _check(lib().smo_timing_select(self._h, mask))
            return
        _check(lib().smo_timing_enable(self._h, (2 + int(only)) if only is not None else (1 if on else 0)))

    def timing(self):
        res = []
        for k in range(lib().smo_timing_classes(self._h)):
            name = C.c_char_p()
            n = C.c_longlong()
            ms = C.c_double()
            by = C.c_double()
            _check(lib().smo_timing_get(self._h, k, C.byref(name), C.byref(n), C.byref(ms), C.byref(by)))
            hb = C.c_double()
            _check(lib().smo_timing_hbm_bytes(self._h, k, C.byref(hb)))
            res.append({"kernel": name.value.decode(), "launches": n.value, "total_ms": ms.value, "bytes_per_launch": by.value,
                        "hbm_bytes_per_launch": hb.value})
        return res


class MultiContext(Context):
    """smo_create_multi: ONE process, ONE context, a KDYN problem slab-decomposed over `devices` (include/smo.h).  forward / adjoint / inner take
    and return the reference's FULL flat vectors like the single-GPU Context; forward_dev / adjoint_dev take one slab pointer per (component,
    device), component-major."""

    def __init__(self, npts, interval, dt, n_iters, Rm, devices, cost="Final", ckpt=1):
        cfg = smo_config(SMO_KDYN, int(npts), float(interval[0]), float(interval[1]), float(dt), int(n_iters), float(Rm),
                         COST[cost] if isinstance(cost, str) else int(cost), 1, int(devices[0]), 0, 1, int(ckpt), 0, 0., 0., 0.)
        self.devices = [int(d) for d in devices]
        ids = (C.c_int * len(self.devices))(*self.devices)
        self._create(cfg, lambda c, h: lib().smo_create_multi(c, len(self.devices), ids, h))

    def _check_dev(self, vecs, who):
        """Per-device slab pointers, component-major: ncomp * ndev of them.  A slab of the wrong length or on the wrong device would be a GPU
        memory fault inside a worker thread, not an exception: every slab that describes itself (DeviceVector, torch tensor) is
        checked; raw integer addresses are the caller's business, as across the C-ABI."""
        nd = len(self.devices)
        want = (2 if who == "inner" else self.ncomp) * nd
        if len(vecs) != want:
            raise ValueError("%s: %d slab pointers given, %d components x %d devices expected" % (who, len(vecs), self.ncomp, nd))
        n_slab = self.vec_len // nd
        for k, v in enumerate(vecs):
            if v is None:
                raise ValueError("%s: slab pointer %d is None" % (who, k))
            if isinstance(v, int):
                continue
            n, idx = _describe_vec(v, who)
            if n is not None and n != n_slab:
                raise ValueError("%s: slab %d has %d entries, the context expects %d (= vec_len / %d devices)" % (who, k, n, n_slab, nd))
            if idx is not None and idx != self.devices[k % nd]:
                raise ValueError("%s: slab %d lives on device %d, rank %d of the context on device %d" % (who, k, idx, k % nd, self.devices[k % nd]))

    # -- vectors that stay distributed over the devices (devvec.MultiDeviceVector): no PCIe traffic, no host algebra on full-size vectors --------
    @staticmethod
    def _on_device(v):
        return hasattr(v, "slabs")

    def _slab_ptrs(self, X):
        for x in X:
            if [s.device for s in x.slabs] != self.devices or sum(s.n for s in x.slabs) != self.vec_len:
                raise ValueError("MultiDeviceVector does not match the context (devices %s, %d entries)" % (self.devices, self.vec_len))
        return [s for x in X for s in x.slabs]                 # component-major: X[c * ndev + i]

    def forward_any(self, X):
        return self.forward_dev(self._slab_ptrs(X)) if self._on_device(X[0]) else self.forward(X)

    def adjoint_any(self, X, adjoint_type="Discrete"):
        if X is not None and len(X) and self._on_device(X[0]):
            from .devvec import MultiDeviceVector
            grads = [MultiDeviceVector.like(X[0]) for _ in range(self.ncomp)]
            self.adjoint_dev(None, self._slab_ptrs(grads), adjoint_type)
            return grads
        return self.adjoint(None, adjoint_type)

    def inner_any(self, x, y):
        dx, dy = self._on_device(x), self._on_device(y)
        if dx != dy:
            raise TypeError("inner product: one operand is a MultiDeviceVector and the other is not")
        if not dx:
            return self.inner(x, y)
        self._slab_ptrs([x, y])
        out = np.zeros(1)
        _check(lib().smo_inner_slabs(self._h, _ptr_array([_dev_ptr(s) for s in x.slabs]), _ptr_array([_dev_ptr(s) for s in y.slabs]),
                                     out.ctypes.data_as(C.POINTER(C.c_double))))
        return float(out[0])
