"""Checkpoint interval of the Poiseuille contexts, host-side checks (no GPU): the domain hands its interval to every context it creates."""
import pytest

from spheremanopt_amd import _capi, poiseuille as pz


class _Recorder:
    made = []

    def __init__(self, kind, npts, interval, dt, n_iters, param, **kw):
        self.kind, self.npts, self.n_iters, self.kw, self.batch = kind, npts, n_iters, kw, kw.get("batch", 1)
        _Recorder.made.append(self)

    def close(self):
        pass


@pytest.mark.parametrize("continuous", [False, True])
def test_domain_passes_its_interval_to_every_context(continuous, monkeypatch):
    monkeypatch.setattr(_capi, "Context", _Recorder)
    _Recorder.made = []
    dom = pz.PoiseuilleDomain(24, 24, continuous=continuous, ckpt=4)
    assert dom.ckpt == 4
    c1 = dom.context(500., 0.05, 9, 5e-3, 0, 1., 0.3)
    c2 = dom.context(500., 0.05, 9, 5e-3, 1, 1., 0.3)
    assert dom.context(500., 0.05, 9, 5e-3, 0, 1., 0.3) is c1          # the interval belongs to the domain, not to the key
    assert [c.kw["ckpt"] for c in _Recorder.made] == [4, 4] and c2 is _Recorder.made[1]
    assert c1.kind == _capi.SMO_POIS and c1.kw["cost"] == (2 if continuous else 0)


def test_default_is_keep_all(monkeypatch):
    monkeypatch.setattr(_capi, "Context", _Recorder)
    _Recorder.made = []
    dom = pz.PoiseuilleDomain(24, 24)
    dom.context(500., 0.05, 3, 5e-3, 0, 1., 0.3)
    assert dom.ckpt == 1 and _Recorder.made[0].kw["ckpt"] == 1
