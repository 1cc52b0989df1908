"""The default fp32 layer-0 kernel (k_pileup_l0_rsx) after its step loop was stripped to the matrix work and the cell (shift-only
staging map, one split-level read, H0 stored straight from the cell's registers: docs/rounds/r13.md) computes, bit for bit, what it
computed before: tests/golden/l0_rsx_parent.npz holds the gt / zy of the parent commit's library on an MI355X for the seeded
inputs of tests/manual/record_l0_parent.py."""
import numpy as np
import pytest

from tests.helpers import golden
from tests.manual.record_l0_parent import SIZES, cases, digest, forward

pytestmark = pytest.mark.gpu

NAMES = [f"n{n}" for n in SIZES] + ["windows50", "big48"]


@pytest.fixture(scope="module")
def recorded():
    return np.load(golden("l0_rsx_parent.npz"))


@pytest.fixture(scope="module")
def inputs():
    c = cases()
    assert sorted(c) == sorted(NAMES)
    return c


@pytest.fixture(scope="module")
def ctx(pileup_weights):
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    c.pileup_load_weights(pileup_weights)
    yield c
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_bits_of_the_parent(name, recorded, inputs, ctx):
    a, b = inputs[name]
    assert digest(a, b) == str(recorded[name + "_sha256"]), "the seeded input is not the one the fixture was recorded for"
    g, z = forward(ctx, a, b)
    assert g.dtype == np.float32 and g.shape == recorded[name + "_gt"].shape and z.shape == recorded[name + "_zy"].shape
    assert np.array_equal(g, recorded[name + "_gt"]) and np.array_equal(z, recorded[name + "_zy"])
