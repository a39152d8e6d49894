"""<robot>.clearance_batch / clearance_batch_multi / planning.path_clearance on the device against the float64 geometry of
tests/geom64.py (used unchanged), evaluated on the product's own fk_batch output for the same configurations (fk_batch
is pinned bit for bit to the golden FK elsewhere).  The minimum is taken FLAT over (fine sphere, contact) and over the
fine self pairs, as include/vamp_mvt_amd.h defines it - not with the gate `max` of geom64.clearances.

BOUND = 2e-5 m for both values.  Coordinates in these scenes stay below 4 m, where one fp32 ulp is 4.8e-7 m; a clearance
is a chain of about a dozen roundings of differences, dot products, one sqrt and the radii: a few micrometres, and the
bound leaves a factor of about four.  Every test prints the largest deviation it saw (pytest -s shows it); on an MI355X
the largest over all robots and scenes was 1.3e-7 m (env) and 5.6e-8 m (self), so the bound could be tightened a
hundredfold."""
import ctypes
import functools

import numpy as np
import pytest

import envs
import geom64

pytestmark = pytest.mark.gpu

ROBOTS = ("panda", "ur5", "fetch", "baxter")
BOUND = 2e-5
BAND = 1e-4  # the sign test's band: five times the value bound (a condition, not a measurement)
BATCHES = (1, 63, 64, 65, 257)  # partial waves, a partial workgroup, more than one tile (tiles hold 64 or 32 configurations)
NONE = np.uint32(0xFFFFFFFF)
KINDS = ("spheres", "capsules", "z_capsules", "cuboids", "z_cuboids")  # witness kinds 0..4 (host_tables names); 5 = heightfield
BORDER = 1e-5


# ---- scenes --------------------------------------------------------------------------------------------------
def coarse_heightfield(robot):
    """the heightfield of envs.spec_for("heightfield"), every 8th pixel: 6 x 6 cells of 0.4 m, so that few spheres lie
    within BORDER of a cell border (with the 5 cm cells of the original, 5 - 9 % of the configurations have one), and
    moved a little in x, y: Fetch's torso spheres stand at y = -0.05 in every configuration, on a border of the original"""
    centre, scale, xd, yd, data = envs.spec_for("heightfield", robot)[-1][1]
    img = np.asarray(data, np.float32).reshape(yd, xd)[::8, ::8]
    centre = (np.asarray(centre, np.float32) + np.array([0.017, 0.011, 0.0], np.float32)).astype(np.float32)
    scale = np.array([scale[0] * 8, scale[1] * 8, scale[2]], np.float32)
    return "heightfield", (centre, scale, img.shape[1], img.shape[0], np.ascontiguousarray(img).reshape(-1))


@functools.lru_cache(maxsize=None)
def scene(robot, kind):
    if kind == "six":  # at least one contact of each of the six kinds
        return tuple(envs.counted_spec(robot, (5, 4, 3, 4, 3), seed=5) + [coarse_heightfield(robot)])
    if kind == "many":  # 150 spheres and 100 z-cuboids: lists longer than a wave
        return tuple(envs.spec_for("many", robot))
    if kind == "heightfield":
        return (coarse_heightfield(robot),)
    if kind in KINDS:  # seven contacts of one kind alone
        counts = [0] * 5
        counts[KINDS.index(kind)] = 7
        return tuple(envs.counted_spec(robot, tuple(counts), seed=9))
    return tuple(envs.spec_for(kind, robot))  # "cage", "mixed", "empty"


# ---- the float64 reference -------------------------------------------------------------------------------------
def contact_columns(spec):
    """-> (tables, [(kind, index)] in the order of the tie rule: kind, then position in the kind's sorted list)"""
    tables = envs.build_product_env(list(spec)).host_tables()
    hfs = geom64.env_parts(list(spec))[0]["heightfield"]
    cols = [(k, i) for k, name in enumerate(KINDS) for i in range(len(tables[name]))] + [(5, i) for i in range(len(hfs))]
    return tables, hfs, cols


def env_matrix(tables, hfs, c, r):
    """float64 clearance of m spheres to every contact -> [m][contacts], columns as contact_columns orders them"""
    parts = []
    if len(tables["spheres"]):
        parts.append(geom64.sphere_clearance(c, r, tables["spheres"]))
    for name in ("capsules", "z_capsules"):
        if len(tables[name]):
            parts.append(geom64.capsule_clearance(c, r, tables[name]))
    for name in ("cuboids", "z_cuboids"):
        if len(tables[name]):
            parts.append(geom64.cuboid_clearance(c, r, tables[name], name == "z_cuboids"))
    parts += [geom64.heightfield_clearance(c, r, h) for h in hfs]
    return np.concatenate(parts, axis=1) if parts else np.zeros((len(c), 0))


def self_pairs(vamp, robot):
    from vamp_mvt_amd import _lib

    rid = getattr(vamp, robot)._id
    n = ctypes.c_size_t(0)
    assert _lib.lib.vmv_robot_self_pairs(rid, ctypes.byref(n), None) == 0
    pairs = np.zeros((n.value, 2), np.uint16)
    assert _lib.lib.vmv_robot_self_pairs(rid, ctypes.byref(n), pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))) == 0
    return pairs.astype(np.int64)


def reference(spec, pairs, fk):
    """fk: float32 [n][spheres][4] (the product's fk_batch) -> dict of float64 arrays: env [n][spheres][contacts] (or None
    without contacts), self [n][pairs], and the (kind, index) of every env column"""
    tables, hfs, cols = contact_columns(spec)
    s = fk.astype(np.float64)
    n, ns = s.shape[:2]
    env = None
    if cols:
        env = np.concatenate([env_matrix(tables, hfs, s[i:i + 32, :, :3].reshape(-1, 3), s[i:i + 32, :, 3].reshape(-1))
                              for i in range(0, n, 32)]).reshape(n, ns, len(cols))
    pa, pb = s[:, pairs[:, 0]], s[:, pairs[:, 1]]
    self_ = geom64._norm(pa[..., :3] - pb[..., :3]) - (pa[..., 3] + pb[..., 3])  # the pair form of geom64.clearances
    return dict(env=env, self=self_, cols=np.array(cols, np.int64).reshape(-1, 2), hfs=hfs)


def border_free(ref, fk):
    """bool[n]: no fine sphere of the configuration lies within BORDER of a heightfield cell border - the heightfield
    value (a step function of the centre) is the same with the centre moved by BORDER towards each corner"""
    s = fk.astype(np.float64)
    n, ns = s.shape[:2]
    c, r = s[..., :3].reshape(-1, 3), s[..., 3].reshape(-1)
    ok = np.ones(n, bool)
    for hf in ref["hfs"]:
        base = geom64.heightfield_clearance(c, r, hf)
        for dx in (-BORDER, BORDER):
            for dy in (-BORDER, BORDER):
                moved = geom64.heightfield_clearance(c + np.array([dx, dy, 0.0]), r, hf)
                ok &= (moved == base).reshape(n, ns).all(axis=1)
    return ok


def flat_minimum(ref):
    """-> (env [n], env argmin as flat (sphere * contacts + column) [n], self [n], self argmin [n]); ties: the first"""
    n = len(ref["self"])
    if ref["env"] is None:
        env, env_at = np.full(n, np.inf), np.full(n, -1)
    else:
        flat = ref["env"].reshape(n, -1)
        env_at = flat.argmin(axis=1)
        env = flat[np.arange(n), env_at]
    self_at = ref["self"].argmin(axis=1)
    return env, env_at, ref["self"][np.arange(n), self_at], self_at


def second_smallest(a, at):
    b = a.copy()
    b[np.arange(len(a)), at] = np.inf
    return b.min(axis=1)


def check_against_reference(ref, fk, values, witness, label):
    """the Values and Witness properties for one batch; -> the largest deviations (env, self) and how many configurations
    the heightfield border rule excluded (the caller holds that against its 2 % cap)"""
    n = len(values)
    env, env_at, self_, self_at = flat_minimum(ref)
    keep = border_free(ref, fk)
    with np.errstate(invalid="ignore"):  # (inf - inf where neither side has a contact)
        dev_env = np.where(np.isinf(env) & np.isinf(values[:, 0]), 0.0, np.abs(values[:, 0].astype(np.float64) - env))[keep]
    dev_self = np.abs(values[:, 1].astype(np.float64) - self_)
    worst = (float(dev_env.max()) if len(dev_env) else 0.0, float(dev_self.max()), int((~keep).sum()))
    print(f"{label}: n = {n}, {worst[2]} excluded, largest deviation env {worst[0]:.3e} m, self {worst[1]:.3e} m")
    assert worst[0] <= BOUND and worst[1] <= BOUND, label
    # witness: in range, its own float64 clearance within BOUND of the float64 minimum, and the float64 argmin wherever the
    # runner-up is more than 2 * BOUND away
    n_pairs = ref["self"].shape[1]
    assert (witness[:, 3] < n_pairs).all(), label
    w_self = ref["self"][np.arange(n), witness[:, 3]]
    assert (np.abs(w_self - self_) <= BOUND).all(), label
    clear = second_smallest(ref["self"], self_at) - self_ > 2 * BOUND
    assert (witness[clear, 3] == self_at[clear]).all(), label
    if ref["env"] is None:
        assert (witness[:, :3] == NONE).all(), label
        return worst
    ns, nc = ref["env"].shape[1:]
    cols = ref["cols"]
    assert (witness[:, 0] < ns).all() and (witness[:, 1] <= 5).all(), label
    col = np.full(n, -1)
    for j, (k, i) in enumerate(cols):
        col[(witness[:, 1] == k) & (witness[:, 2] == i)] = j
    assert (col >= 0).all(), f"{label}: a witnessed (kind, index) names no contact of the scene"
    w_env = ref["env"][np.arange(n), witness[:, 0], col]
    assert (np.abs(w_env - env) <= BOUND)[keep].all(), label
    flat = ref["env"].reshape(n, -1)
    clear = (second_smallest(flat, env_at) - env > 2 * BOUND) & keep
    assert ((witness[:, 0].astype(np.int64) * nc + col)[clear] == env_at[clear]).all(), label
    return worst


def halton(vamp, robot, n, skip):
    return getattr(vamp, robot).halton_device(n, skip).cpu().numpy()


# ---- values and witness ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["six", "many"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_values_and_witness_match_float64(vamp, robot, kind):
    mod = getattr(vamp, robot)
    spec = scene(robot, kind)
    env = envs.build_product_env(list(spec))
    pairs = self_pairs(vamp, robot)
    skip, worst = 0, (0.0, 0.0, 0)
    for n in BATCHES:
        q = halton(vamp, robot, n, skip)
        skip += n
        fk = mod.fk_batch(q)
        assert np.abs(fk[..., :3]).max() < 4.0  # the bound's premise
        values, witness = mod.clearance_batch(q, env, witness=True)
        assert values.shape == (n, 2) and values.dtype == np.float32 and witness.shape == (n, 4) and witness.dtype == np.uint32
        assert np.array_equal(values, mod.clearance_batch(q, env))  # the witness does not change the values
        w = check_against_reference(reference(spec, pairs, fk), fk, values, witness, f"{robot} {kind} n={n}")
        worst = (max(worst[0], w[0]), max(worst[1], w[1]), worst[2] + w[2])
    print(f"{robot} {kind}: largest deviation over all batches env {worst[0]:.3e} m, self {worst[1]:.3e} m (bound {BOUND:.0e})")
    assert worst[2] <= 0.02 * sum(BATCHES), f"{worst[2]} of {sum(BATCHES)} configurations excluded at cell borders"


@pytest.mark.parametrize("kind", KINDS + ("heightfield",))
def test_each_kind_alone(vamp, kind):
    """every distance form on its own, so that none hides behind a smaller value of another kind"""
    spec = scene("panda", kind)
    env = envs.build_product_env(list(spec))
    q = halton(vamp, "panda", 65, 1000)
    fk = vamp.panda.fk_batch(q)
    values, witness = vamp.panda.clearance_batch(q, env, witness=True)
    assert (witness[:, 1] == (KINDS + ("heightfield",)).index(kind)).all()
    w = check_against_reference(reference(spec, self_pairs(vamp, "panda"), fk), fk, values, witness, f"panda {kind} alone")
    assert w[2] <= 0.02 * len(q)


def test_single_configuration_call(vamp):
    env = envs.build_product_env(list(scene("panda", "six")))
    q = halton(vamp, "panda", 3, 77)
    values = vamp.panda.clearance_batch(q, env)
    for i in range(3):
        got = vamp.panda.clearance(q[i], env)
        assert isinstance(got[0], float) and np.array_equal(np.array(got, np.float32), values[i])


# ---- the sign agrees with validation ---------------------------------------------------------------------------------
# The batches: the first 512 Halton samples have at least 20 % of the configurations on each side and at most 2 % inside
# the band for every robot and scene but Panda in the cage (17 % valid), whose last 128 are replaced by configurations
# around the cage example's start.  The test checks it with the oracle's validate_batch and the float64 minimum.
def sign_batch(vamp, robot, kind):
    from oracle_lib import CAGE_START

    q = halton(vamp, robot, 512, 0)
    if (robot, kind) == ("panda", "cage"):
        q[384:] = (np.asarray(CAGE_START, np.float32) + np.random.default_rng(0).normal(0, 0.3, (128, 7))).astype(np.float32)
    return q


@pytest.mark.parametrize("kind", ["cage", "mixed"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_sign_agrees_with_validate_batch(vamp, oracle, robot, kind):
    mod = getattr(vamp, robot)
    spec = scene(robot, kind)
    env = envs.build_product_env(list(spec))
    q = sign_batch(vamp, robot, kind)
    n = len(q)
    # the batch is the kind the test asks for: judged on the CPU by the oracle and the float64 minimum
    rid = oracle.robot(robot)
    valid = oracle.validate_batch(rid, envs.build_oracle_env(oracle, list(spec)), q).astype(bool)
    fk = np.stack([oracle.fk(rid, qi) for qi in q])
    env64, _, self64, _ = flat_minimum(reference(spec, self_pairs(vamp, robot), fk))
    in_band = np.abs(np.minimum(env64, self64)) < BAND
    assert valid.mean() >= 0.2 and (~valid).mean() >= 0.2 and in_band.mean() <= 0.02, (valid.mean(), in_band.mean())
    values = mod.clearance_batch(q, env)
    least = values.min(axis=1)
    judged = np.abs(least) >= np.float32(BAND)
    got = mod.validate_batch(q, env)
    print(f"{robot} {kind}: {valid.mean():.2f} valid, {int((~judged).sum())} of {n} inside the band")
    assert np.array_equal(got[judged], least[judged] > 0)


# ---- independence, multi, edge cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_configuration_does_not_depend_on_its_batch(vamp, robot):
    mod = getattr(vamp, robot)
    env = envs.build_product_env(list(scene(robot, "six")))
    q = halton(vamp, robot, 300, 5000)
    probe = q[17].copy()
    alone_v, alone_w = mod.clearance_batch(probe[None, :], env, witness=True)
    for n, at in ((64, 0), (64, 63), (65, 64), (130, 129), (257, 256), (300, 31), (300, 32)):
        batch = q[:n].copy()
        batch[at] = probe
        v, w = mod.clearance_batch(batch, env, witness=True)
        assert np.array_equal(v[at].view(np.uint32), alone_v[0].view(np.uint32)) and np.array_equal(w[at], alone_w[0]), (n, at)


@pytest.mark.parametrize("robot", ROBOTS)
def test_multi_equals_single_calls_bit_for_bit(vamp, robot):
    import torch

    mod = getattr(vamp, robot)
    scenes = [envs.build_product_env(list(scene(robot, k))) for k in ("six", "many", "mixed")]
    counts = [0, 65, 1]
    q = halton(vamp, robot, 66, 9000)
    values, witness = mod.clearance_batch_multi(q, scenes, counts, witness=True)
    assert values.shape == (66, 2) and witness.shape == (66, 4)
    v1, w1 = mod.clearance_batch(q[:65], scenes[1], witness=True)
    v2, w2 = mod.clearance_batch(q[65:], scenes[2], witness=True)
    assert np.array_equal(values.view(np.uint32), np.concatenate([v1, v2]).view(np.uint32))
    assert np.array_equal(witness, np.concatenate([w1, w2]))
    assert np.array_equal(mod.clearance_batch_multi(q, scenes, counts).view(np.uint32), values.view(np.uint32))
    # several segments of more than one tile, with a None among them
    counts = [100, 7, 130, 20]
    q = halton(vamp, robot, 257, 9100)
    values, witness = mod.clearance_batch_multi(q, [scenes[2], None, scenes[0], scenes[2]], counts, witness=True)
    lo = 0
    for e, c in zip([scenes[2], vamp.Environment(), scenes[0], scenes[2]], counts):
        v, w = mod.clearance_batch(q[lo:lo + c], e, witness=True)
        assert np.array_equal(values[lo:lo + c].view(np.uint32), v.view(np.uint32)) and np.array_equal(witness[lo:lo + c], w)
        lo += c
    # the device entry points (torch CUDA tensors in and out) agree with the host ones bit for bit
    qt = torch.from_numpy(q).cuda()
    vt, wt = mod.clearance_batch_multi(qt, [scenes[2], None, scenes[0], scenes[2]], counts, witness=True)
    assert np.array_equal(vt.cpu().numpy().view(np.uint32), values.view(np.uint32))
    assert np.array_equal(wt.cpu().numpy().view(np.uint32), witness)
    vt, wt = mod.clearance_batch(qt[:100], scenes[2], witness=True)
    assert np.array_equal(vt.cpu().numpy().view(np.uint32), values[:100].view(np.uint32))
    assert np.array_equal(wt.cpu().numpy().view(np.uint32), witness[:100])


@pytest.mark.parametrize("robot", ROBOTS)
def test_without_an_environment_and_in_an_empty_one(vamp, robot):
    mod = getattr(vamp, robot)
    q = halton(vamp, robot, 70, 300)
    fk = mod.fk_batch(q)
    ref = reference((), self_pairs(vamp, robot), fk)
    v_none, w_none = mod.clearance_batch(q, None, witness=True)
    v_empty, w_empty = mod.clearance_batch(q, vamp.Environment(), witness=True)
    for v, w in ((v_none, w_none), (v_empty, w_empty)):
        assert (v[:, 0] == np.inf).all() and (w[:, :3] == NONE).all()
    assert np.array_equal(v_none.view(np.uint32), v_empty.view(np.uint32)) and np.array_equal(w_none, w_empty)
    check_against_reference(ref, fk, v_none, w_none, f"{robot} without an environment")
    # the self clearance does not depend on the environment
    v_six = mod.clearance_batch(q, envs.build_product_env(list(scene(robot, "six"))))
    assert np.array_equal(v_six[:, 1].view(np.uint32), v_none[:, 1].view(np.uint32))


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_non_finite_joint_gives_nan_and_leaves_its_neighbours_alone(vamp, robot):
    mod = getattr(vamp, robot)
    env = envs.build_product_env(list(scene(robot, "six")))
    q = halton(vamp, robot, 130, 700)
    clean_v, clean_w = mod.clearance_batch(q, env, witness=True)
    bad = q.copy()
    rows = [0, 5, 63, 64, 129]
    for j, i in enumerate(rows):
        bad[i, j % q.shape[1]] = (np.nan, np.inf, -np.inf)[j % 3]
    v, w = mod.clearance_batch(bad, env, witness=True)
    assert np.isnan(v[rows]).all() and (w[rows] == NONE).all()
    others = np.setdiff1d(np.arange(130), rows)
    assert np.array_equal(v[others].view(np.uint32), clean_v[others].view(np.uint32)) and np.array_equal(w[others], clean_w[others])
    v2, w2 = mod.clearance_batch_multi(bad, [env, None], [100, 30], witness=True)
    assert np.isnan(v2[rows]).all() and (w2[rows] == NONE).all()


def test_path_clearance_equals_per_sample_calls(vamp):
    from vamp_mvt_amd.planning import path_clearance, path_samples

    mod = vamp.panda
    scenes = [envs.build_product_env(list(scene("panda", k))) for k in ("cage", "mixed")]
    q = halton(vamp, "panda", 4, 40).astype(np.float64)
    paths = [np.stack([q[0], q[0] + 0.04 * (q[1] - q[0]), q[0] + 0.1 * (q[1] - q[0])]),
             np.stack([q[2], q[2] + 0.07 * (q[3] - q[2])])]
    got = path_clearance(mod, paths, scenes)
    for p, e, g in zip(paths, scenes, got):
        samples, at = path_samples(p, mod.resolution())
        assert len(samples) > len(p)
        v = np.concatenate([mod.clearance_batch(s[None, :], e) for s in samples])
        ie, js = int(v[:, 0].argmin()), int(v[:, 1].argmin())
        assert g.env == float(v[ie, 0]) and g.env_at == tuple(at[ie]) and g.self_ == float(v[js, 1]) and g.self_at == tuple(at[js])
