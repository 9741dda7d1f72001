"""Batched Poiseuille contexts, host-side checks (no GPU): what is refused before any device is touched."""
import pytest

from spheremanopt_amd import poiseuille as pz


def test_batch_must_be_positive():
    dom = pz.PoiseuilleDomain(24, 24)
    with pytest.raises(ValueError):
        dom.context(500., 0.05, 2, 5e-3, 0, 1., 0.3, batch=0)
    assert dom._ctx == {}


def test_batch_on_a_continuous_domain_is_refused_before_any_device_call():
    dom = pz.PoiseuilleDomain(16, 16, continuous=True)
    with pytest.raises(ValueError, match="Discrete"):
        dom.context(500., 0.05, 2, 5e-3, 0, 1., 0.3, batch=2)
    assert dom._ctx == {}
