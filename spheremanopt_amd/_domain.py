"""What the problem modules share on the Python side: the context cache of a ``domain`` and the handle to the HBM snapshot stack."""


class DomainBase:
    """Owner of the device contexts of one geometry, one per parameter set.  A subclass sets its geometry, gives `context` its
    problem's positional signature and supplies `_make_context(*key, batch)`, `_DEFAULT` and the names of further contexts it opens."""
    _DEFAULT = ()            # parameters of the one-step context any_context() creates when no batch-1 context is cached
    _EXTRA = ()              # attributes that hold contexts outside the cache (None until opened)

    def __init__(self):
        self._ctx = {}

    def context(self, *key, batch=1):
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch = %d: at least one member" % batch)
        key += (batch,)
        if key not in self._ctx:
            self._ctx[key] = self._make_context(*key)
        return self._ctx[key]

    def any_context(self):
        """A batch-1 context (the inner products and transforms of the reference-signature callables act on single vectors): a cached
        one, else a one-step context made for the purpose."""
        for c in self._ctx.values():
            if c.batch == 1:
                return c
        return self.context(*self._DEFAULT)

    def drop_contexts(self):
        """Close every context now: each owns its whole HBM snapshot stack, which would otherwise wait for the garbage collector."""
        for c in self._ctx.values():
            c.close()
        self._ctx = {}
        for name in self._EXTRA:
            if getattr(self, name, None) is not None:
                getattr(self, name).close()
                setattr(self, name, None)


class SnapshotStack:
    """Handle to device-resident snapshots (an X_FWD_DICT entry of GEN_BUFFER): ``stack[..., i]`` reads snapshot i from HBM; negative i
    count from the end.  `decode(ctx, i)` returns the array the leading part of the key indexes; `solver` names the forward solve that
    fills the stack."""

    def __init__(self, shape, decode, solver):
        self.shape, self.decode, self.solver, self.ctx = shape, decode, solver, None

    def __getitem__(self, key):
        if self.ctx is None:
            raise RuntimeError("snapshot stack is empty: run %s first" % self.solver)
        idx = key[-1]
        return self.decode(self.ctx, idx + self.shape[-1] if idx < 0 else idx)[key[:-1]]


def attach(X_FWD_DICT, ctx):
    """Point every stack of a GEN_BUFFER dictionary at the context whose forward solve has just filled it."""
    for stack in X_FWD_DICT.values():
        stack.ctx = ctx
