"""The CPU oracle's direct-light term held to the float64 closed form of tests/light_ref.py, and two properties
of that term on a builtin scene.  The oracle is a float32 restatement written beside the kernels; light_ref.py is
written from the formulas alone, so a shared misreading (a directional light's sign, the cosine the BRDF carries,
the attenuation constants, the shadow ray's interval) shows here as an error far above float32 rounding.

The light term is acc(light) - acc(no light) of a depth-1, 1-spp frame: lights never steer a path, so the two
renders trace the same closest-hit rays and differ by the light's contribution alone."""
import numpy as np
import pytest

import light_common as LC
import light_ref
import oracle


@pytest.fixture(scope="module")
def ref_setup():
    cam = oracle.camera(LC.CAM_POS, LC.CAM_TARGET_REF, aspect=LC.W / LC.H)
    dirs, _ = oracle.primary(cam, LC.W, LC.H, 1)
    return cam, dirs, oracle.Prepared(LC.ref_scene(), bvh=True)


def oracle_light_term(P, cam, mats, lights, w=LC.W, h=LC.H, **kw):
    lit, _, c1 = P.render(cam, w, h, mats, LC.light_rows(lights), threads=LC.THREADS, **kw)
    dark, _, c0 = P.render(cam, w, h, mats, LC.light_rows([]), threads=LC.THREADS, **kw)
    return lit - dark, c1, c0


@pytest.mark.parametrize("light", list(LC.REF_LIGHTS))
@pytest.mark.parametrize("mat", list(LC.REF_MATS))
def test_oracle_light_term_against_float64(ref_setup, mat, light):
    cam, dirs, P = ref_setup
    row = LC.REF_MATS[mat]
    got, c1, c0 = oracle_light_term(P, cam, np.stack([row, row]), [LC.REF_LIGHTS[light]], max_depth=1)
    ref = light_ref.direct_light(cam[:3], dirs, row, row, LC.REF_LIGHTS[light])
    m = LC.against_ref(got, ref)
    print(f"{mat} {light}: d_case {m['rel_l1']:.3e} excluded {m['excluded_share']:.5f} {m}")
    assert c1["rays_closest"] == c0["rays_closest"] == LC.W * LC.H and c0["rays_shadow"] == 0
    facing = int(ref["facing"].sum())  # one shadow ray per hit the light is in front of (the suite's count rule)
    assert abs(c1["rays_shadow"] - facing) <= 1e-3 * facing + 5, (c1["rays_shadow"], facing)
    LC.check_ref_case(m, LC.d_ceiling(mat), (mat, light))


def test_light_term_is_additive_and_order_independent():
    """default_emitter, 4 spp, depth 6: the SUN+POINT light term is the sum of the two single-light terms up to the
    order of float32 additions (measured 4.2e-8 relative L1; asserted with a 4x margin), and swapping the two
    lights changes it by 2.7e-9 (again 4x); the closest-hit ray count does not depend on the lights."""
    P = oracle.Prepared(oracle.builtin_scene("default_emitter"), bvh=True)
    cam = oracle.camera(LC.CAM_POS, LC.CAM_TARGET, aspect=LC.W / LC.H)
    mats = oracle.preset_materials(True)
    terms, closest = {}, set()
    for name in ("SUN", "POINT", "SUN+POINT", "POINT+SUN"):
        terms[name], c1, c0 = oracle_light_term(P, cam, mats, name, frames=4)
        closest |= {c1["rays_closest"], c0["rays_closest"]}
        assert c0["rays_shadow"] == 0 and c1["rays_shadow"] > 0
    both = terms["SUN+POINT"].astype(np.float64)
    add = LC.rel_l1(terms["SUN"].astype(np.float64) + terms["POINT"], both)
    order = LC.rel_l1(terms["POINT+SUN"], terms["SUN+POINT"])
    lit = float((both != 0).any(axis=2).mean())
    print(f"additivity residue {add:.3e}, order residue {order:.3e}, lit share {lit:.3f}, rays_closest {closest}")
    assert len(closest) == 1
    assert lit >= 0.25
    assert add <= 4 * 4.2e-8, add
    assert order <= 4 * 2.7e-9, order
