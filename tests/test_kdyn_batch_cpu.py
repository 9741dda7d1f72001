"""Batched KDyn contexts, host-side checks (no GPU): what is refused before any device is touched."""
import pytest

from spheremanopt_amd import kdyn


def test_batch_on_a_multi_device_domain_is_refused_before_any_device_call():
    dom = kdyn.KDynDomain(16, devices=[0, 0])
    with pytest.raises(ValueError, match="one GPU"):
        dom.context(1., 1e-3, 2, "Final", batch=2)
    assert dom._ctx == {}


def test_batch_must_be_positive():
    dom = kdyn.KDynDomain(16)
    with pytest.raises(ValueError):
        dom.context(1., 1e-3, 2, "Final", batch=0)
    assert dom._ctx == {}
