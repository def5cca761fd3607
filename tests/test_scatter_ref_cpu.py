"""CPU: the float64 scatter model (tests/scatter_ref.py) and what the GPU scatter tests (tests/test_gpu_scatter.py)
rely on, without a device.

The oracle's float32 trace_path renders every ray set of scatter_common through the sets' cameras; every pixel the
model does not flag as fragile must be within half of the model's bound where the bound is derived, and the
oracle's closest-hit count must be the model's segment count.  Where the bound is not derived (a sphere hit from
a computed origin) the oracle's worst needed du is what the GPU tests grant 4 x of.  The model flags at most 1 % of
any set, every branch is taken by at least 2 % of some set, and fifteen deliberately wrong variants of the model
each put the oracle at least ten bounds away on the set aimed at them.  Measures are printed as `SCATTER_MEASURE`
lines (profiles/scatter_measurements.txt)."""
import numpy as np
import pytest

import adversarial_common as A
import residue
import scatter_common as SC
import scatter_ref as R

ORACLE_MAX_RATIO = 0.5
MAX_FRAGILE = 0.01
MIN_BRANCH_SHARE = 0.02
MUTANT_MIN_RATIO = 10.0
ENV_IDS = [f"{kind}{S}" for S, kind, _ in SC.ENVS]
# the set each mutant is aimed at
MUTANT_SETS = {
    "sincos_swapped": "diffuse", "b_is_cross_n_t": "diffuse", "onb_never_switched": "diffuse", "sqrt_swapped": "diffuse",
    "xi_first": "diffuse", "roulette_from_2": "slab", "roulette_no_division": "slab", "eta_is_ior": "glass_panels",
    "schlick_x4": "glass_panels", "tr_unclamped": "glass_panels", "refract_origin_plus": "glass",
    "fresnel_reflect_times_tr": "glass_panels", "metal_albedo_only": "metal", "emission_after": "slab",
    "no_face_forward": "glass_panels",
}


def _worst(r, keep):
    return float(r[keep].max()) if keep.any() else 0.0


# ---- the sets -----------------------------------------------------------------------------------------------------
def test_scenes_are_what_they_claim():
    t, _ = A.staging_counts()
    for name, (_, n_staged, n_unstaged) in SC.SCENES.items():
        sc = SC.scene(name)
        for N, staged in ((n_staged, True), (n_unstaged, False)):
            flat = SC.flat_scene(sc, N)
            nt, ns = len(flat["indices"]), len(flat["spheres"])
            assert nt == 2 * N * N * len(sc["rects"]) and len(flat["geom_material"]) == len(sc["rects"]) + ns
            assert (A.staged_bytes(nt + ns, nt, ns, nt + ns) <= A.header_constant("kLdsSceneBytes")) == staged, (name, N)
            assert (nt <= t) == staged
    m = SC.PROBE_MATERIALS
    assert m[3, 8] > np.float32(1.3) and m[8, 8] == np.float32(1.3) and m[9, 3] == np.float32(0.1)
    assert 0.9499 < (np.float64(m[5, 8]) - 1) / R.C_07 < R.C_095 <= (np.float64(m[6, 8]) - 1) / R.C_07
    nz = {o: abs(np.cross(*SC.ORIENT[o])[2]) / np.linalg.norm(np.cross(*SC.ORIENT[o])) for o in ("tilt_lo", "tilt_hi")}
    assert nz["tilt_lo"] < 0.999 - 5 * R.NZ_MARGIN and nz["tilt_hi"] > 0.999 + 5 * R.NZ_MARGIN
    assert set(o for o, _ in SC.PANELS) == set(SC.ORIENT) and set(range(13)) == set(mat for _, mat in SC.PANELS)


@pytest.mark.parametrize("name", SC.SET_NAMES + SC.FRAME_NAMES)
def test_set_sizes_and_fragile_share(name):
    rs = SC.ray_set(name)
    assert 2000 <= len(rs) <= 10000 and rs.dirs.dtype == np.float32 and rs.states.dtype == np.uint32
    for e in range(len(SC.ENVS)):
        for depth in (1, 2, 3, SC.MAX_DEPTH):
            share = float(rs.model(e, depth)["fragile"].mean())
            print(f"SCATTER_MEASURE model fragile set={name} env={ENV_IDS[e]} depth={depth} n={len(rs)} share={share:.5f}")
            assert share <= MAX_FRAGILE, (name, e, depth, share)


def test_incidence_runs_from_normal_to_grazing():
    """The probe sets' first hits: incidence below 2 degrees and above 89.9 degrees both occur on either side."""
    for name in ("metal", "glass_panels", "diffuse"):
        rs = SC.ray_set(name)
        res = rs.model(0, 1)
        cos = np.full(len(rs), np.nan)
        for p, u, v, _ in SC.scene("probes")["rects"]:
            nh = np.cross(u, v) / np.linalg.norm(np.cross(u, v))
            d = rs.dirs.astype(np.float64)
            t = ((p - rs.origins) @ nh) / (d @ nh)
            q = rs.origins + t[:, None] * d - p
            inside = (t > 0) & (q @ u > 0) & (q @ u < u @ u) & (q @ v > 0) & (q @ v < v @ v) & np.isnan(cos)
            cos = np.where(inside, d @ nh, cos)
        for side in (1, -1):
            c = -side * cos[(res["kind"][:, 0] != R.NONE) & (side * cos < 0)]
            deg = np.degrees(np.arccos(np.clip(c, 0, 1)))
            print(f"set {name} side {side}: incidence {deg.min():.3f} .. {deg.max():.3f} degrees over {len(deg)} hits")
            assert deg.min() < 2.0 and deg.max() > 89.9, (name, side, deg.min(), deg.max())


def test_every_branch_is_taken():
    """From the model's branch record at full depth: each branch's largest share of the rays of a set."""
    best = {}
    for name in SC.SET_NAMES:
        res = SC.ray_set(name).model(0)
        kind, share = res["kind"], {}
        share["mirror"] = (kind == R.MIRROR).any(axis=1).mean()
        share["fresnel_reflect"] = (kind == R.FRESNEL).any(axis=1).mean()
        share["refract"] = (kind == R.REFRACT).any(axis=1).mean()
        share["diffuse_z"] = (kind == R.DIFFUSE_Z).any(axis=1).mean()
        share["diffuse_y"] = (kind == R.DIFFUSE_Y).any(axis=1).mean()
        share["roulette_kill"] = (res["rr"] == R.RR_KILL).any(axis=1).mean()
        share["roulette_survive"] = (res["rr"] == R.RR_SURVIVE).any(axis=1).mean()
        share["emission_at_bounce_1_or_later"] = res["emit"][:, 1:].any(axis=1).mean()
        share["back_side_hit"] = res["back"].any(axis=1).mean()
        share["inside_refraction"] = ((kind == R.REFRACT) & res["back"]).any(axis=1).mean()
        for k, v in share.items():
            if v > best.get(k, (0.0, ""))[0]:
                best[k] = (float(v), name)
    for k, (v, name) in best.items():
        print(f"SCATTER_MEASURE model branch {k} share={v:.4f} set={name}")
    assert len(best) == 10 and all(v >= MIN_BRANCH_SHARE for v, _ in best.values()), best
    # roulette is met at every bounce index it applies to, and the glass spheres are gone through to the depth
    slab = SC.ray_set("slab").model(0)
    for b in (3, 4, 5):
        assert (slab["rr"][:, b] == R.RR_KILL).mean() >= 0.02 and (slab["rr"][:, b] == R.RR_SURVIVE).mean() >= 0.02, b
    assert (slab["rr"][:, :3] == R.RR_NONE).all()
    assert (SC.ray_set("glass").model(0)["segments"] == SC.MAX_DEPTH).mean() >= 0.02


# ---- the bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.SET_NAMES + SC.FRAME_NAMES)
@pytest.mark.parametrize("e", range(len(SC.ENVS)), ids=ENV_IDS)
def test_oracle_within_the_bound(name, e):
    rs = SC.ray_set(name)
    for depth in (1, 2, 3, SC.MAX_DEPTH):
        got, closest = rs.oracle(e, depth)
        res = rs.model(e, depth)
        assert np.isfinite(got).all()
        keep = ~res["fragile"]
        # (a fragile path may take other branches: up to depth - 1 segments more or fewer; the drawn sets have none)
        assert abs(closest - int(res["segments"].sum())) <= (depth - 1) * int((~keep).sum()), (name, depth, closest)
        assert keep.all() or name in SC.FRAME_NAMES
        derived = keep & ~res["underived"]
        r = R.ratio(got, res)
        du, need = rs.granted_du(e, depth)
        rb = R.ratio(got, rs.bound(e, depth))
        rec = {"set": name, "env": ENV_IDS[e], "depth": depth, "n": len(rs), "fragile": int((~keep).sum()),
               "underived": int((keep & res["underived"]).sum()), "oracle_worst_ratio_derived": round(_worst(r, derived), 4),
               "oracle_needed_du_eps": round(need / R.EPS, 2), "granted_du_eps": round(du / R.EPS, 2),
               "oracle_worst_ratio_granted": round(_worst(rb, keep), 4)}
        residue.log_parity(f"SCATTER_MEASURE oracle {name} {ENV_IDS[e]} depth={depth}", rec)
        k = int(np.argmax(np.where(derived, r, 0)))
        assert r[k] <= ORACLE_MAX_RATIO or not derived[k], (name, depth, rs.dirs[k], got[k], res["value"][k], res["tol"][k])
        assert np.isfinite(need)
        # exactly 0 where the path uses up the depth without emission
        ended = keep & (res["segments"] == depth) & (res["value"] == 0).all(axis=1) & (res["env_scale"] == 0).all(axis=1)
        assert (got[ended] == 0).all()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    """A misreading of the reference exceeds the bound by an order of magnitude or more on the set aimed at it: the
    (right) oracle against each wrong variant of the model, through the measure the real comparison uses."""
    rs = SC.ray_set(MUTANT_SETS[mutant])
    worst, share = 0.0, 0.0
    for e in range(len(SC.ENVS)):
        got, _ = rs.oracle(e)
        res = rs.model(e, mutant=mutant, du_underived=rs.granted_du(e)[0])
        keep = ~(res["fragile"] | rs.model(e)["fragile"])
        r = R.ratio(got, res)[keep]
        worst, share = max(worst, float(r.max())), max(share, float((r > 1.0).mean()))
    residue.log_parity(f"SCATTER_MEASURE mutant {mutant}", {"set": rs.name, "worst_ratio": float(f"{worst:.3g}"),
                                                            "share_outside": round(share, 4)})
    assert worst >= MUTANT_MIN_RATIO, (mutant, worst)
