"""The Python front end without the library or a GPU: the context cache every domain inherits from _domain.DomainBase, the snapshot
handle, and SlabDomain's solver cache.  _capi.Context / _capi.MultiContext are replaced by a stub that records what it is asked."""
import types

import numpy as np
import pytest

from spheremanopt_amd import _capi, _domain, kdyn, kdyn_slab, sh23, shb23
from spheremanopt_amd import poiseuille as pz


class StubContext:
    def __init__(self, *args, **kw):
        self.args, self.kw, self.batch = args, kw, int(kw.get("batch", 1))
        self.closed, self.reads, self.snapshot_len = False, [], 0
        self.made.append(self)

    def close(self):
        self.closed = True

    def forward_any(self, X):
        return -1.0

    def snapshot(self, index, b=0):
        self.reads.append(index)
        return np.arange(self.snapshot_len, dtype=np.float64) + index

    def transform(self, which, x, out_len=None):
        return np.zeros(out_len)


@pytest.fixture
def made(monkeypatch):
    """Every context created during the test, in order."""
    stub = type("Stub", (StubContext,), {"made": []})
    monkeypatch.setattr(_capi, "Context", stub)
    monkeypatch.setattr(_capi, "MultiContext", stub)
    return stub.made


# name -> (domain factory, positional arguments of context(), another value for each of them)
DOMAINS = {
    "sh23": (lambda: sh23.SH23Domain(64), (0.1, 4), (0.2, 5)),
    "shb23": (lambda: shb23.SHBDomain(64), (1e-2, 4), (2e-2, 5)),
    "kdyn": (lambda: kdyn.KDynDomain(16), (1., 1e-3, 2, "Final"), (2., 2e-3, 3, "Integrated")),
    "poiseuille": (lambda: pz.PoiseuilleDomain(24, 24), (500., 0.05, 2, 5e-3, 0, 1., 0.3), (400., 0.06, 3, 4e-3, 1, 2., 0.25)),
}
each_domain = pytest.mark.parametrize("name", sorted(DOMAINS))


@each_domain
def test_any_context_is_batch_1_whatever_was_cached_first(made, name):
    new, args, _ = DOMAINS[name]
    dom = new()
    assert dom.context(*args, batch=3).batch == 3 and len(made) == 1
    c = dom.any_context()
    assert c.batch == 1 and c is made[-1] and len(made) == 2          # exactly one context more
    assert dom.any_context() is c and len(made) == 2                  # and it is reused
    assert dom.context(*args, batch=3) is made[0]


@each_domain
def test_any_context_prefers_a_cached_batch_1_context(made, name):
    new, args, _ = DOMAINS[name]
    dom = new()
    c = dom.context(*args)
    assert dom.any_context() is c and len(made) == 1


@each_domain
def test_cache_is_keyed_by_every_parameter(made, name):
    new, args, other = DOMAINS[name]
    dom = new()
    c = dom.context(*args)
    assert dom.context(*args) is c and dom.context(*args, batch=1) is c and len(made) == 1
    seen = [c]
    for i in range(len(args)):
        changed = args[:i] + (other[i],) + args[i + 1:]
        d = dom.context(*changed)
        assert all(d is not s for s in seen), i
        assert dom.context(*changed) is d
        seen.append(d)
    b = dom.context(*args, batch=2)
    assert b.batch == 2 and all(b is not s for s in seen) and dom.context(*args, batch=2) is b
    assert len(made) == len(args) + 2 and len(dom._ctx) == len(made)


def test_kdyn_default_cost_shares_the_context_of_final(made):
    dom = kdyn.KDynDomain(16)
    assert dom.context(1., 1e-3, 2) is dom.context(1., 1e-3, 2, "Final") and len(made) == 1


@each_domain
def test_batch_0_is_refused(made, name):
    new, args, _ = DOMAINS[name]
    dom = new()
    with pytest.raises(ValueError):
        dom.context(*args, batch=0)
    assert dom._ctx == {} and made == []


@each_domain
def test_drop_contexts_closes_everything(made, name):
    new, args, other = DOMAINS[name]
    dom = new()
    dom.context(*args, batch=3)
    dom.context(*other, batch=2)
    dom.any_context()
    if name == "kdyn":
        kdyn._coeff3_to_grid(dom, np.zeros((3, dom.a, dom.m, dom.m), dtype=complex))
        assert dom._transform_ctx is made[-1] and dom._transform_ctx not in dom._ctx.values()
    assert len(made) == (4 if name == "kdyn" else 3) and not any(c.closed for c in made)
    dom.drop_contexts()
    assert all(c.closed for c in made) and dom._ctx == {}
    if name == "kdyn":
        assert dom._transform_ctx is None
    n = len(made)
    assert dom.context(*args, batch=3) is made[-1] and len(made) == n + 1 and not made[-1].closed      # usable again


@pytest.mark.parametrize("in_library", [True, False])
def test_slab_domain_drops_its_solvers_contexts(monkeypatch, made, in_library):
    def lib_solver(*a, **kw):
        return types.SimpleNamespace(ctx=_capi.Context())

    def phase_solver(*a, **kw):
        return types.SimpleNamespace(ops=types.SimpleNamespace(ctx=_capi.Context()))
    monkeypatch.setattr(kdyn_slab, "LibSlabKDyn", lib_solver)
    monkeypatch.setattr(kdyn_slab, "SlabKDyn", phase_solver)
    dom = kdyn_slab.SlabDomain(16, in_library=in_library)
    s1 = dom.solver(1., 1e-3, 2)
    s2 = dom.solver(1., 1e-3, 3, "Integrated")
    assert dom.solver(1., 1e-3, 2, "Final") is s1 and dom.any_solver() is s1 and s2 is not s1 and len(made) == 2
    dom.drop_contexts()
    assert all(c.closed for c in made) and dom._solvers == {}


def _solved(name, n):
    """(stacks, stub context) after a forward solve of n steps through the module's own callback."""
    dom = DOMAINS[name][0]()
    x = [np.zeros(4)]
    if name == "sh23":
        buf = sh23.GEN_BUFFER(dom, n)
        call = lambda: sh23.FWD_Solve_IVP_Lin(x, dom, 0.1, n, n, buf)                      # noqa: E731
        length = 2 * dom.Nc
    elif name == "shb23":
        buf = shb23.GEN_BUFFER(64, dom, n)
        call = lambda: shb23.FWD_Solve_IVP_Discrete(x, dom, buf, n, 1e-2)                  # noqa: E731
        length = dom.Npts
    elif name == "kdyn":
        buf = kdyn.GEN_BUFFER(16, dom, n)
        call = lambda: kdyn.FWD_Solve_IVP_Lin(x + x, dom, 1., 1e-3, n, n, buf)             # noqa: E731
        length = 2 * 3 * dom.a * dom.m * dom.m
    else:
        buf = pz.GEN_BUFFER(24, 24, dom, n)
        call = lambda: pz.FWD_Solve_Discrete(x, dom, 500., 0.05, n, buf, 5e-3)             # noqa: E731
        length = 2 * 3 * dom.a * dom.Nz
    return dom, buf, call, length


@each_domain
def test_snapshot_stack_is_empty_before_a_forward_solve(made, name):
    _, buf, _, _ = _solved(name, 5)
    solver = {"sh23": "FWD_Solve_IVP_Lin", "shb23": "FWD_Solve_IVP_Discrete", "kdyn": "FWD_Solve_IVP_Lin", "poiseuille": "FWD_Solve_Discrete"}
    for stack in buf.values():
        assert isinstance(stack, _domain.SnapshotStack) and stack.ctx is None
        with pytest.raises(RuntimeError, match="snapshot stack is empty: run %s first" % solver[name]):
            stack[(slice(None),) * (len(stack.shape) - 1) + (0,)]


@each_domain
def test_snapshot_stack_decodes_like_the_reference_buffers(made, name):
    n = 5
    dom, buf, call, length = _solved(name, n)
    assert call() == -1.0 and len(made) == 1
    ctx = made[0]
    ctx.snapshot_len = length
    raw = lambda i: np.arange(length, dtype=np.float64) + i                               # noqa: E731
    if name == "sh23":
        assert list(buf) == ['A_fwd'] and buf['A_fwd'].shape == (dom.Nc, n + 1)
        want = {'A_fwd': lambda i: raw(i).view(np.complex128)}
        keys = [(slice(None),), (slice(1, 5),), (3,)]
    elif name == "shb23":
        assert list(buf) == ['A_fwd'] and buf['A_fwd'].shape == (dom.Npts, n + 1)
        want = {'A_fwd': raw}
        keys = [(slice(None),), (slice(1, 5),), (3,)]
    elif name == "kdyn":
        a, m = dom.a, dom.m
        assert list(buf) == ['A_fwd', 'B_fwd', 'C_fwd'] and all(s.shape == (a, m, m, n + 1) for s in buf.values())
        want = {k: (lambda i, c=c: raw(i).view(np.complex128).reshape(3, a, m, m)[c]) for c, k in enumerate(buf)}
        keys = [(slice(None),) * 3, (1, slice(None), 2), (slice(2, 4), 0, slice(None, None, 2))]
    else:
        a, Nz = dom.a, dom.Nz
        assert list(buf) == ['u_fwd', 'w_fwd', 'b_fwd'] and all(s.shape == (a, Nz, n + 1) for s in buf.values())
        want = {k: (lambda i, f=f: raw(i).view(np.complex128).reshape(3, a, Nz)[f]) for f, k in enumerate(buf)}
        keys = [(slice(None),) * 2, (1, slice(None)), (slice(2, 4), 5)]
    for k, stack in buf.items():
        assert stack.ctx is ctx
        for key in keys:
            for i, read in ((0, 0), (2, 2), (n, n), (-1, n), (-2, n - 1)):
                got = stack[key + (i,)]
                assert ctx.reads[-1] == read                                   # index -1 reads snapshot shape[-1] - 1
                ref = want[k](read)[key]
                assert np.shape(got) == np.shape(ref) and np.array_equal(got, ref), (k, key, i)
