"""Slab-decomposed kinematic dynamo over the GPUs of one node: one process per GPU, RCCL all-to-all pencil transposes.

Parallel layout (the reference gets the same decomposition implicitly from Dedalus' MPI layouts):
  * coefficient space is split over kx   (rank r owns kx in [r*a/W, (r+1)*a/W))  -> the z pass and the per-mode solves are local
  * grid space is split over z           (rank r owns z  in [r*G/W, (r+1)*G/W))  -> the y and x passes and all grid products are local
  * between the z and the y pass ONE all-to-all per direction per step, carrying all fields of that direction at once, at the point
    where the data is smallest (16*a*m*G bytes per component; after the y pass it would be 16*a*G*G, 1.5x more); the device
    kernels write/read the exchange buffers as [peer][field group][3][a/W][m][G/W], i.e. contiguous per peer.
  * when the HBM allows it the forward solve keeps B_n on the y side (after exchange and y pass) for every step, so an adjoint step
    exchanges omega only on its inverse side; the adjoint's second product (the dJ/dU forcing) is summed over the steps on the grid
    side and transformed once at the end: 4 field-group exchanges per forward+adjoint step pair (fwd 1+1, adj 1+1) instead of 6.
  * scalars (J, <x,y>) are all-reduced; the snapshot stack (1/W of it per GPU), the per-mode solves and the
    products need no communication.

The time loop only *enqueues* work: the device phases (``smo_kdyn_op``) and the collectives run on the same HIP stream
(torch's current stream), so there is no host synchronisation inside a solve with the NCCL(=RCCL) backend.

`SlabKDyn.forward / adjoint / inner` work on LOCAL slabs ([3][G][G][G/W] float64 tensors on the device).
The module-level callables keep the reference's replicated-vector semantics (FWD_Solve_KDyn.py:91-171: every rank holds the
full vectors; gradients are all-gathered), so ``Optimise_On_Multi_Sphere`` runs unchanged, redundantly on every rank.
"""
import os

import numpy as np

from . import _capi
from ._capi import (SMO_KD_SET_BUFFERS as SET_BUFFERS, SMO_KD_EXCHANGE_ELEMS as EXCHANGE_ELEMS, SMO_KD_G2C_A as G2C_A, SMO_KD_G2C_C as G2C_C,
                    SMO_KD_C2G_A as C2G_A, SMO_KD_C2G_B as C2G_B, SMO_KD_FWD_A as FWD_A, SMO_KD_FWD_B as FWD_B, SMO_KD_FWD_C as FWD_C,
                    SMO_KD_ENERGY as ENERGY, SMO_KD_ADJ_INIT as ADJ_INIT, SMO_KD_ADJ_A as ADJ_A, SMO_KD_ADJ_B as ADJ_B, SMO_KD_ADJ_C as ADJ_C,
                    SMO_KD_SYNC as SYNC, SMO_KD_SET_CHUNKS as SET_CHUNKS, SMO_KD_NU_B as NU_B, SMO_KD_NU_C as NU_C)
from .kdyn import check_interval


def _dist():
    import torch.distributed as dist
    return dist


def rank_world():
    try:
        dist = _dist()
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


class HipOps:
    """Device phases through the C-ABI (the product path)."""

    def __init__(self, Npts, Rm, dt, N_ITERS, Cost_function, device, rank, world, stream=None):
        import ctypes as C
        self._C = C
        self.ctx = _capi.Context(_capi.SMO_KDYN, Npts, (0., 2. * np.pi), dt, N_ITERS, Rm, cost=Cost_function, device=device,
                                 rank=rank, world=world)
        self.lib = _capi.lib()
        if stream is not None:
            _capi._check(self.lib.smo_set_stream(self.ctx._h, C.c_void_p(stream)))
        out = C.c_double()
        self.op(EXCHANGE_ELEMS, out=out)
        self.elems = int(out.value)
        self.vec_len = self.ctx.vec_len

    def op(self, code, i0=0, p0=None, p1=None, out=None, i1=0):
        C = self._C
        ref = C.byref(out) if out is not None else None
        _capi._check(self.lib.smo_kdyn_op(self.ctx._h, code, int(i0), int(i1), C.c_void_p(p0), C.c_void_p(p1), ref))

    def set_chunks(self, K):
        self.op(SET_CHUNKS, K)

    def set_buffers(self, zs, ys):
        self.op(SET_BUFFERS, p0=zs.data_ptr(), p1=ys.data_ptr())

    @property
    def keeps_grid_states(self):
        """True when the forward solve keeps B_n on the y side (the adjoint's inverse exchange then carries one field group)."""
        return self.ctx.get(1) > 0

    def energy(self, n):
        out = self._C.c_double()
        self.op(ENERGY, n, out=out)
        return out.value

    def dot(self, x, y):
        return self.ctx.inner_dev(x, y)

    def phase(self, code, i0=0, vec=None, k=0):
        self.op(code, i0, p0=(vec.data_ptr() if vec is not None else None), i1=k)

    def sync(self):
        self.op(SYNC)

    def snapshot(self, n):
        return self.ctx.snapshot(n)


class _Slab:
    """What the two slab solvers share: this rank's place in the decomposition, the yes/no agreement across the ranks and the
    replicated-vector helpers.  A solver adds `dev` (its torch device) and `host_staged` (collectives go through host tensors)."""

    def __init__(self, Npts):
        import torch
        self.torch = torch
        self.rank, self.world = rank_world()
        self.N, self.G = int(Npts), 3 * int(Npts) // 2
        if (self.N // 2) % self.world or self.G % self.world:
            raise ValueError("%d slabs do not divide a=%d / G=%d" % (self.world, self.N // 2, self.G))
        self.Gzl = self.G // self.world

    def _all_ranks(self, flag, op, device):
        """Collective: `flag` of every rank reduced with "MIN" (true on all ranks?) or "MAX" (true on any rank?)."""
        dist = _dist()
        t = self.torch.tensor([1.0 if flag else 0.0], dtype=self.torch.float64, device="cpu" if dist.get_backend() == "gloo" else device)
        dist.all_reduce(t, op=getattr(dist.ReduceOp, op))
        return float(t.item()) > 0.5

    # -- replicated-vector helpers (the reference's Vec_to_Field / Field_to_Vec across ranks) ------------------------------------
    def local_slab(self, full):
        """Full flat vector [3][G][G][G] (NumPy or tensor, any device) -> this rank's z-slab as a flat device tensor."""
        G, z0 = self.G, self.rank * self.Gzl
        t = self.torch.as_tensor(np.asarray(full, dtype=np.float64) if not self.torch.is_tensor(full) else full)
        return t.reshape(3, G, G, G)[:, :, :, z0:z0 + self.Gzl].contiguous().reshape(-1).to(self.dev)

    def gather_full(self, local):
        """Local slab -> full flat NumPy vector on every rank (all-gather over z)."""
        G = self.G
        loc = local.reshape(3, G, G, self.Gzl)
        if self.world == 1:
            return loc.reshape(-1).cpu().numpy()
        dist = _dist()
        staged = self.host_staged or self.dev.type == "cpu"
        src = loc.cpu().contiguous() if staged else loc.contiguous()
        parts = [self.torch.empty_like(src) for _ in range(self.world)]
        dist.all_gather(parts, src)
        return self.torch.cat(parts, dim=3).reshape(-1).cpu().numpy()


class SlabKDyn(_Slab):
    """One rank's share of the forward / adjoint solve.  `ops` is the phase backend (HipOps unless a test injects its own)."""

    def __init__(self, Npts, Rm, dt, N_ITERS, Cost_function="Final", device=None, ops=None, stage_through_host=None, chunks=None):
        super().__init__(Npts)
        torch = self.torch
        self.Rm, self.dt, self.n_iters, self.cost = float(Rm), float(dt), int(N_ITERS), Cost_function
        self.stream = None
        if ops is None:
            if device is None:
                device = torch.cuda.current_device()
            self.dev = torch.device("cuda", device)
            with torch.cuda.device(self.dev):
                self.stream = torch.cuda.Stream()            # kernels AND collectives are ordered on this stream
            ops = HipOps(Npts, Rm, dt, N_ITERS, Cost_function, device, self.rank, self.world, stream=self.stream.cuda_stream)
            if self.world > 1:
                # whether the grid-side states are kept decides how many field groups an adjoint step exchanges: every rank takes that
                # decision from its own free HBM, so agree on it (all or none) before the first collective of a solve could mismatch
                everyone = self._all_ranks(ops.keeps_grid_states, "MIN", self.dev)
                if ops.keeps_grid_states and not everyone:
                    ops.ctx.close()
                    prev = os.environ.get("SMO_KD_TYSTACK")
                    os.environ["SMO_KD_TYSTACK"] = "0"
                    try:
                        ops = HipOps(Npts, Rm, dt, N_ITERS, Cost_function, device, self.rank, self.world, stream=self.stream.cuda_stream)
                    finally:
                        if prev is None:
                            del os.environ["SMO_KD_TYSTACK"]
                        else:
                            os.environ["SMO_KD_TYSTACK"] = prev
        else:
            self.dev = torch.device(getattr(ops, "device", "cpu"))
        self.ops = ops
        self.elems = ops.elems                                  # complex128 per field group, all peers
        # exchange buffers as float64 pairs (RCCL has no complex type): 2 field groups x elems complex128
        # SMO_SLAB_FORCE_EXCHANGE=1: keep the two sides apart and run the collective even on ONE rank (a self-copy through the process
        # group) — lets a single-GPU box exercise the real RCCL call path (stream ordering, buffer views) of the multi-GPU loop
        self.force_exchange = (self.world == 1 and os.environ.get("SMO_SLAB_FORCE_EXCHANGE", "0") == "1" and
                               _dist().is_available() and _dist().is_initialized())
        self.buf_z = torch.zeros(4 * self.elems, dtype=torch.float64, device=self.dev)      # z-pass side (kx slab, all z)
        self.buf_y = self.buf_z if (self.world == 1 and not self.force_exchange) else torch.zeros_like(self.buf_z)   # y-pass side (all kx, z slab)
        ops.set_buffers(self.buf_z, self.buf_y)
        self.adj_groups = 1 if ops.keeps_grid_states else 2
        # pipelining: the local z slab is cut into K chunks; the all-to-all of chunk k overlaps the grid-side kernels of the other chunks
        # (the collectives run on the process group's own stream, the kernels on the solver's).  Default: up to 4 chunks of at least 9216
        # (y,z) points each — below that the grid-side kernels become launch-bound and chunking costs more than it hides (measured on
        # one rank, profiles/r01_rccl_one_rank.jsonl).
        if chunks is None:
            chunks = int(os.environ.get("SMO_SLAB_CHUNKS", "0")) or (max(1, min(4, (self.G * self.Gzl) // 9216)) if self.world > 1 else 1)
        while chunks > 1 and (self.Gzl % chunks or (self.Gzl // chunks) % 2 or (self.G * (self.Gzl // chunks)) % 4):
            chunks -= 1
        self.K = chunks
        if self.K > 1:
            ops.set_chunks(self.K)
        backend = _dist().get_backend() if (self.world > 1 or self.force_exchange) else None
        # collectives on device tensors need RCCL; with gloo (CPU tests, or several ranks sharing one GPU) stage through the host
        self.host_staged = (self.dev.type == "cuda" and backend == "gloo") if stage_through_host is None else stage_through_host
        self.have_forward = False
        self._views = {}

    # -- communication -----------------------------------------------------------------------------------------------
    def _exchange(self, src, dst, nfields, k=0, wait=True):
        """All-to-all of chunk k (nfields field groups) from `src` to `dst`.  With RCCL the collective is enqueued on the process
        group's stream behind everything already on the solver's stream; `wait=False` returns the work handle so that kernels
        enqueued next (on other chunks) overlap it — call `_wait(handle)` before the first kernel that reads `dst`."""
        if self.world == 1 and not self.force_exchange:
            return None
        key = (src is self.buf_z, nfields, k)
        views = self._views.get(key)
        if views is None:                                       # the views are cached: slicing costs microseconds, this runs 4x per step pair
            n = 2 * nfields * self.elems // self.K              # float64 words of this chunk
            c0 = k * (4 * self.elems // self.K)                 # chunks are spaced for two field groups whatever `nfields` is
            views = self._views[key] = (src[c0:c0 + n], dst[c0:c0 + n])
        s_, d_ = views
        dist = _dist()
        if self.host_staged:
            self.ops.sync()
            h = s_.cpu()
            r = self.torch.empty_like(h)
            dist.all_to_all_single(r, h)
            d_.copy_(r)
            return None
        if wait:
            dist.all_to_all_single(d_, s_)
            return None
        return dist.all_to_all_single(d_, s_, async_op=True)

    @staticmethod
    def _wait(work):
        if work is not None:
            work.wait()                                         # stream-level: the solver's stream waits, the host does not

    def _grid_stage(self, code, i0, to_y, to_z, nf_in, nf_out):
        """One transpose -> grid work -> transpose back, chunk-pipelined: z-side -> y-side, phase `code` per chunk, y-side -> z-side."""
        if self.K == 1:
            self._exchange(to_y[0], to_y[1], nf_in)
            self.ops.phase(code, i0)
            self._exchange(to_z[0], to_z[1], nf_out)
            return
        inbound = [self._exchange(to_y[0], to_y[1], nf_in, k, wait=False) for k in range(self.K)]
        outbound = []
        for k in range(self.K):
            self._wait(inbound[k])
            self.ops.phase(code, i0, k=k)
            outbound.append(self._exchange(to_z[0], to_z[1], nf_out, k, wait=False))
        for w in outbound:
            self._wait(w)

    def _allreduce(self, value):
        if self.world == 1:
            return float(value)
        dev = "cpu" if (self.host_staged or self.dev.type == "cpu") else self.dev
        t = self.torch.tensor([value], dtype=self.torch.float64, device=dev)
        _dist().all_reduce(t)
        return float(t.item())

    # -- transforms of whole vectors ------------------------------------------------------------------------------------
    def _grid_to_coeff(self, vec, target):
        for k in range(self.K):
            self.ops.phase(G2C_A, vec=vec, k=k)
            self._exchange(self.buf_y, self.buf_z, 1, k)
        self.ops.phase(G2C_C, target)

    def _coeff_to_grid(self, source, vec):
        self.ops.phase(C2G_A, source)
        for k in range(self.K):
            self._exchange(self.buf_z, self.buf_y, 1, k)
            self.ops.phase(C2G_B, vec=vec, k=k)

    # -- the three callbacks on local slabs --------------------------------------------------------------------------------
    def _on_stream(self):
        """Context manager: make the solver's stream current (inputs produced on the caller's stream are waited for)."""
        import contextlib
        if self.stream is None:
            return contextlib.nullcontext()
        self.stream.wait_stream(self.torch.cuda.current_stream(self.dev))
        return self.torch.cuda.stream(self.stream)

    def _done(self):
        if self.stream is not None:
            self.torch.cuda.current_stream(self.dev).wait_stream(self.stream)

    def forward(self, X):
        """X = [B_local, U_local]; returns -J (identical on every rank)."""
        with self._on_stream():
            J = self._forward(X)
        self._done()
        return J

    def adjoint(self, Adjoint_type="Discrete", out=None):
        """[dJ/dB0 local slab, dJ/dU local slab]; replays the snapshots of the last forward()."""
        with self._on_stream():
            g = self._adjoint(Adjoint_type, out)
        self._done()
        return g

    def _forward(self, X):
        B, U = X[0], X[1]
        self.have_forward = False
        self._grid_to_coeff(U, 1)             # U^ (truncated) -> scratch
        self._coeff_to_grid(1, None)          # scratch -> the context's grid field U
        self._grid_to_coeff(B, 0)             # B^_0 -> snapshot 0
        integ = self.cost == "Integrated"
        J = 0.0
        for n in range(self.n_iters):
            if integ:
                J += self.dt * self.ops.energy(n)
            self.ops.phase(FWD_A, n)                       # z pass (inverse)
            # transpose, then y, x passes, U x B on the grid, x, y passes back, transpose back (chunk-pipelined)
            self._grid_stage(FWD_B, n, (self.buf_z, self.buf_y), (self.buf_y, self.buf_z), 1, 1)
            self.ops.phase(FWD_C, n)                       # z pass (forward) + curl, projection, CNAB1 update
        E = self.ops.energy(self.n_iters)
        J = J + self.dt * E if integ else E
        self.have_forward = True
        return -self._allreduce(J)

    def _adjoint(self, Adjoint_type="Discrete", out=None):
        if not self.have_forward:
            raise RuntimeError("adjoint() needs forward() first (it replays that snapshot stack)")
        cont = Adjoint_type == "Continuous"
        self.ops.phase(ADJ_INIT, _capi.ADJOINT[Adjoint_type])
        idx = self.n_iters if cont else self.n_iters - 1
        for _ in range(self.n_iters):
            self.ops.phase(ADJ_A, idx)
            self._grid_stage(ADJ_B, idx, (self.buf_z, self.buf_y), (self.buf_y, self.buf_z),
                             self.adj_groups if idx < self.n_iters else 2, 1)
            self.ops.phase(ADJ_C, idx)
            idx -= 1
        # nu^: the second cross product was summed over the steps on the grid side; transform the sum once
        for k in range(self.K):
            self.ops.phase(NU_B, k=k)
            self._exchange(self.buf_y, self.buf_z, 1, k)
        self.ops.phase(NU_C)
        if out is None:
            out = [self.torch.empty(self.ops.vec_len, dtype=self.torch.float64, device=self.dev) for _ in range(2)]
        self._coeff_to_grid(1 if cont else 0, out[0])
        self._coeff_to_grid(2, out[1])
        self.ops.sync()
        return out

    def inner(self, x, y):
        with self._on_stream():
            d = self.ops.dot(x, y)
        self._done()
        return self._allreduce(d)


class LibSlabKDyn(_Slab):
    """One rank's share of the forward / adjoint solve with the time loop AND the transposes inside libsmo (include/smo.h,
    "in-library time loop"): the context is given a communicator once and smo_forward_dev / smo_adjoint_dev / smo_inner_dev are then
    called collectively like their single-GPU forms.  Transport:
      * "rccl" (default with the nccl backend): rank 0 makes an RCCL unique id, torch.distributed only carries those 128 bytes to
        the other ranks, and libsmo opens its own communicator (grouped ncclSend/ncclRecv on the solver's HIP streams);
      * "callback" (default with gloo — ranks sharing a GPU in tests): the library calls back into Python for every exchange, which
        stages the blocks through the host and torch.distributed's all_to_all_single.
    Same local-slab interface as SlabKDyn (forward / adjoint / inner / local_slab / gather_full)."""

    def __init__(self, Npts, Rm, dt, N_ITERS, Cost_function="Final", device=None, ckpt=1, transport=None):
        super().__init__(Npts)
        torch = self.torch
        self.n_iters, self.cost = int(N_ITERS), Cost_function
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        # a rank that cannot build its context (e.g. not enough HBM for its share of the stack) must not leave the others waiting in
        # the communicator's rendezvous: every rank reports, all raise together
        self.ctx, err = None, None
        try:
            self.ctx = _capi.Context(_capi.SMO_KDYN, Npts, (0., 2. * np.pi), dt, N_ITERS, Rm, cost=Cost_function, device=self.device,
                                     rank=self.rank, world=self.world, ckpt=ckpt)
        except Exception as e:               # noqa: BLE001
            err = e
        if self.world > 1 and self._all_ranks(err is not None, "MAX", self.dev) and err is None:
            self.ctx.close()
            err = RuntimeError("LibSlabKDyn: another rank could not create its context")
        if err is not None:
            raise err
        self.vec_len = self.ctx.vec_len
        force = self.world == 1 and os.environ.get("SMO_SLAB_FORCE_EXCHANGE", "0") == "1"
        self.transport = None
        if self.world > 1 or force:
            dist = _dist()
            if transport is None:
                transport = "rccl" if dist.get_backend() == "nccl" else "callback"
            self.transport = transport
            if transport == "rccl":
                box = [_capi.comm_unique_id() if self.rank == 0 else None]
                if self.world > 1:
                    dist.broadcast_object_list(box, src=0)
                self.ctx.comm_init(box[0])
            else:
                self.ctx.comm_set_transport(self._a2a_host_staged, self._allreduce_host)
        self.K = int(self.ctx.comm_get(0)) if self.transport else 1
        self.exchanges_per_step_pair = int(self.ctx.comm_get(1)) if self.transport else 0

    # -- the callback transport: blocks staged through the host, torch.distributed (gloo) in between ----------------------------
    def _a2a_host_staged(self, src, dst, bytes_per_peer, stream):
        import ctypes as C
        torch, L = self.torch, _capi.lib()
        torch.cuda.synchronize(self.dev)                      # the kernels that produced `src` run on the library's own streams
        n = bytes_per_peer * self.world // 8
        h = torch.empty(n, dtype=torch.float64)
        _capi._check(L.smo_vec_download(self.device, C.c_void_p(src), C.c_void_p(h.data_ptr()), n))
        r = torch.empty_like(h)
        if self.world > 1:
            _dist().all_to_all_single(r, h)
        else:
            r.copy_(h)
        _capi._check(L.smo_vec_upload(self.device, C.c_void_p(dst), C.c_void_p(r.data_ptr()), n))

    def _allreduce_host(self, vals, n):
        if self.world == 1:
            return
        t = self.torch.tensor([vals[i] for i in range(n)], dtype=self.torch.float64)
        _dist().all_reduce(t)
        for i in range(n):
            vals[i] = float(t[i])

    def set_chunks(self, K):
        """Collective: cut the local z slab into K pipelined chunks (smo_kdyn_op SMO_KD_SET_CHUNKS); raises if K does not divide it."""
        import ctypes as C
        _capi._check(_capi.lib().smo_kdyn_op(self.ctx._h, SET_CHUNKS, int(K), 0, C.c_void_p(None), C.c_void_p(None), None))
        self.K = int(self.ctx.comm_get(0))

    def autotune_chunks(self, X, candidates=(1, 2, 4)):
        """Collective: time one forward + adjoint solve per candidate chunk count and keep the fastest (slowest rank decides, so every
        rank picks the same).  How well the transposes hide behind the grid-side kernels depends on the xGMI rate of the node, which no
        single-GPU measurement can tell; a few solves at start-up can.  Returns {K: seconds}."""
        import time
        torch, times = self.torch, {}
        out = [torch.empty(self.vec_len, dtype=torch.float64, device=self.dev) for _ in range(2)]
        for K in candidates:
            try:
                self.set_chunks(K)
            except _capi.SmoError:
                continue                                   # K does not divide the slab into even parts
            if self.K != K:
                continue
            self.forward(X); self.adjoint("Discrete", out)  # first run with this K: allocations, communicator warm-up
            torch.cuda.synchronize(self.dev)
            if self.world > 1:
                _dist().barrier()
            t0 = time.perf_counter()
            self.forward(X); self.adjoint("Discrete", out)
            torch.cuda.synchronize(self.dev)
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cpu" if self.host_staged else self.dev)
            if self.world > 1:
                _dist().all_reduce(t, op=_dist().ReduceOp.MAX)
            times[K] = float(t.item())
        if times:
            self.set_chunks(min(times, key=times.get))
        return times

    def _sync_inputs(self):
        self.torch.cuda.current_stream(self.dev).synchronize()     # inputs produced by torch kernels; libsmo runs on its own streams

    def forward(self, X):
        self._sync_inputs()
        return self.ctx.forward_dev([X[0], X[1]])

    def adjoint(self, Adjoint_type="Discrete", out=None):
        if out is None:
            out = [self.torch.empty(self.vec_len, dtype=self.torch.float64, device=self.dev) for _ in range(2)]
        self._sync_inputs()
        self.ctx.adjoint_dev([out[0], out[1]], out, Adjoint_type)
        return out

    def inner(self, x, y):
        self._sync_inputs()
        return self.ctx.inner_dev(x, y)

    @property
    def host_staged(self):
        return self.transport != "rccl"


# ---- the reference's callback surface on top of the slab solver (replicated full vectors in / out) -----------------------------

class SlabDomain:
    """`domain` slot of args_f / args_IP for the multi-GPU run: caches one SlabKDyn per (Rm, dt, N_ITERS, cost)."""

    def __init__(self, Npts, X=(0., 2. * np.pi), device=None, in_library=True, ckpt=1):
        """in_library=True: the time loop and the transposes run inside libsmo (LibSlabKDyn); False: the Python loop over the
        phase-level entry (SlabKDyn, the CPU/gloo test harness)."""
        check_interval(X)
        self.Npts, self.interval, self.device = int(Npts), X, device
        self.G = 3 * self.Npts // 2
        self.hypervolume = (X[1] - X[0]) ** 3
        self.in_library, self.ckpt = in_library, ckpt
        self._solvers = {}

    def solver(self, Rm, dt, N_ITERS, Cost_function="Final"):
        key = (float(Rm), float(dt), int(N_ITERS), Cost_function)
        if key not in self._solvers:
            if self.in_library:
                self._solvers[key] = LibSlabKDyn(self.Npts, Rm, dt, N_ITERS, Cost_function, device=self.device, ckpt=self.ckpt)
            else:
                self._solvers[key] = SlabKDyn(self.Npts, Rm, dt, N_ITERS, Cost_function, device=self.device)
        return self._solvers[key]

    def any_solver(self):
        if not self._solvers:
            self.solver(1., 1e-3, 1)
        return next(iter(self._solvers.values()))

    def drop_contexts(self):
        """Close every solver's context now (collective in effect: each rank drops its share of the HBM snapshot stacks)."""
        for s in self._solvers.values():
            (s.ctx if self.in_library else s.ops.ctx).close()
        self._solvers = {}


def FWD_Solve_IVP_Lin(X0, domain, Rm, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT=None, Cost_function="Final", Adjoint_type="Discrete"):
    s = domain.solver(Rm, dt, N_ITERS, Cost_function)
    return s.forward([s.local_slab(X0[0]), s.local_slab(X0[1])])


def ADJ_Solve_IVP_Lin(X0, domain, Rm, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT=None, Cost_function="Final", Adjoint_type="Discrete"):
    s = domain.solver(Rm, dt, N_ITERS, Cost_function)
    g = s.adjoint(Adjoint_type)
    return [s.gather_full(g[0]), s.gather_full(g[1])]


def Inner_Prod_3(x, y, domain, random_arg=None):
    s = domain.any_solver()
    return s.inner(s.local_slab(x), s.local_slab(y))
