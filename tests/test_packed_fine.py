"""The environment kernels' packed fine phase (vmv_device.h env_fine_packed) vs the oracle, bit for bit: configurations
of all four robots at ragged batch sizes, a dense scene (most lanes pass their gates: full buffers and mid-link flushes
with k up to 64), a sparse one (single passing lanes) and edges (rakes of G = 8)."""
import numpy as np
import pytest

from envs import build_oracle_env, build_product_env, spec_for
from vamp_mvt_amd.workloads import shell_spec

pytestmark = pytest.mark.gpu
ROBOTS = ["panda", "ur5", "fetch", "baxter"]
SIZES = [1, 63, 65, 1000, 4097]


def scenes(name):
    dense = shell_spec(11, 48, 48, 0.3, 0.75)  # primitives all around the arm: most gates fire for most lanes
    sparse = [("sphere", np.array([0.55, 0.1, 0.6, 0.03], np.float32))]  # one small obstacle: a lane here and there
    return dict(dense=dense, sparse=sparse, mixed=spec_for("mixed", name))  # (mixed: general cuboids and capsules too)


def uniform(oracle, name, n, seed):
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(seed)
    return rid, (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)


def check_configs(vamp, oracle, name):
    for si, (kind, spec) in enumerate(scenes(name).items()):
        env, oenv = build_product_env(spec), build_oracle_env(oracle, spec)
        for n in SIZES:
            rid, q = uniform(oracle, name, n, seed=1000 * si + n)
            got = getattr(vamp, name).validate_batch(q, env)
            want = oracle.validate_batch(rid, oenv, q, threads=8)
            assert np.array_equal(got, want), (name, kind, n, int((got != want).sum()))
        if kind == "dense":  # the case must really be dense: few configurations valid
            assert want.mean() < 0.5, want.mean()


def check_edges(vamp, oracle, name):
    for kind, spec in scenes(name).items():
        env, oenv = build_product_env(spec), build_oracle_env(oracle, spec)
        rid, a = uniform(oracle, name, 700, seed=7)
        rng = np.random.default_rng(8)
        b = (a + rng.normal(0, 0.2, a.shape)).astype(np.float32)
        got = getattr(vamp, name).validate_motion_batch(a, b, env)
        want = oracle.validate_motion_batch(rid, oenv, a, b)
        assert np.array_equal(got, want), (name, kind, int((got != want).sum()))


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


@pytest.mark.parametrize("name", ROBOTS)
def test_packed_configs(vamp, oracle, name):
    check_configs(vamp, oracle, name)


@pytest.mark.parametrize("name", ROBOTS)
def test_packed_edges(vamp, oracle, name):
    check_edges(vamp, oracle, name)
