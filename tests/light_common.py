"""Light sets, material rows, scenes and measures shared by test_light_ref_cpu.py and test_gpu_light_parity.py
(test infrastructure, numpy only: scenes are the oracle's dicts, lights and materials its float rows)."""
import os

import numpy as np

import light_ref

THREADS = min(16, os.cpu_count() or 1)
W, H = 96, 64
CAM_POS = (0.0, 2.2, 4.5)
CAM_TARGET = (0.0, 0.6, 0.0)     # the parity renders
CAM_TARGET_REF = (0.0, 0.5, 0.0)  # the float64 cases

# light rows: type, v (direction the light travels / position), colour, intensity
SUN = [0, -0.5, -1.0, 0.3, 1.0, 0.95, 0.8, 2.0]  # the default light
POINT = [1, 1.5, 4.0, 2.0, 1.0, 0.8, 0.6, 30.0]
FILL = [0, 0.6, -1.0, -0.2, 0.4, 0.5, 0.9, 0.7]
LOW = [1, -2.5, 0.3, 1.0, 0.9, 0.9, 1.0, 12.0]   # grazing: 0.3 above the floor
MORE = [[1, -2.5, 0.6, 2.5, 0.9, 0.9, 1.0, 12.0],
        [1, 0.0, 6.0, -3.0, 1.0, 1.0, 1.0, 40.0],
        [0, -1.0, -0.3, 0.1, 0.2, 0.2, 0.2, 1.0],
        [1, 3.0, 1.0, 3.0, 0.5, 1.0, 0.5, 8.0],
        [0, 0.1, -1.0, 0.9, 0.3, 0.1, 0.1, 0.5]]
LIGHT_SETS = {
    "NONE": [],
    "SUN": [SUN],
    "POINT": [POINT],
    "SUN+POINT": [SUN, POINT],
    "POINT+SUN": [POINT, SUN],
    "THREE": [SUN, POINT, FILL],
    "EIGHT": [SUN, POINT, FILL] + MORE,
}


def light_rows(name_or_rows):
    rows = LIGHT_SETS[name_or_rows] if isinstance(name_or_rows, str) else name_or_rows
    return np.array(rows, np.float32).reshape(-1, 8)


def mat_row(albedo=(0.8, 0.6, 0.4), metallic=0.0, roughness=0.5, ior=1.0, emission=(0.0, 0.0, 0.0), type=0):
    m = np.zeros(12, np.float32)
    m[0:3], m[3], m[4], m[5:8], m[8], m[9] = albedo, metallic, roughness, emission, ior, type
    return m


# ---- the float64 cases: one material on both primitives, one light -------------------------------------------
REF_LIGHTS = {"POINT": POINT, "SUN": SUN, "LOW": LOW}
REF_MATS = {
    "r0": mat_row(roughness=0.0),
    "r0.02_ior1.5": mat_row(roughness=0.02, ior=1.5),
    "r0.05": mat_row(roughness=0.05),
    "r0.5": mat_row(roughness=0.5),
    "r1": mat_row(roughness=1.0),
    "m0.4_r0.3_ior1.2": mat_row(metallic=0.4, roughness=0.3, ior=1.2),
    "m0.5_r1": mat_row(metallic=0.5, roughness=1.0),
    "m1_r0.02": mat_row(metallic=1.0, roughness=0.02),
    "m1_r0.3": mat_row(metallic=1.0, roughness=0.3),
    "ior2.4_r0.5": mat_row(ior=2.4, roughness=0.5),
    "black": mat_row(albedo=(0.0, 0.0, 0.0)),
}
# Relative L1 of the float32 oracle's light term against the float64 form, measured per material on the CPU over
# the three lights (the worst of the three is stated): the ceiling the oracle is held to.  The two mirror-like
# metals are the worst: their GGX lobe D = a2 / (pi ((N.H)^2 (a2 - 1) + 1)^2) loses digits where N.H is near 1.
D_CEILING = {"m1_r0.02": 3.9e-5, "m1_r0.3": 1.8e-5}
D_CEILING_REST = 6e-6
FLOOR_EPS = 16.0 * 2.0 ** -23  # no bound below 16 float32 epsilons
EXCLUDE_REL, EXCLUDE_ABS = 1e-4, 1e-3
MAX_EXCLUDED = 0.005


def d_ceiling(mat_name):
    return max(D_CEILING.get(mat_name, D_CEILING_REST), FLOOR_EPS)


def ref_scene():
    """light_ref's scene as the oracle's dict: the floor (geometry 0, material 0), the sphere (1, material 1)."""
    x0, x1 = light_ref.FLOOR_X
    z0, z1 = light_ref.FLOOR_Z
    return {"positions": np.array([[x0, 0, z0], [x1, 0, z0], [x1, 0, z1], [x0, 0, z1]], np.float32),
            "indices": np.array([[0, 2, 1], [0, 3, 2]], np.uint32),
            "tri_geom_first": np.array([0, 2], np.uint32),
            "spheres": np.array([light_ref.SPHERE], np.float32),
            "geom_material": np.array([0, 1], np.uint32)}


def against_ref(got, ref):
    """got (H, W, 3): a float32 light term; ref: light_ref.direct_light's dict.  A hit pixel is excluded when its
    largest channel error exceeds 1e-4 of max(its largest reference channel, 1e-3): shadow-edge and silhouette
    pixels, where a float32 and a float64 hit test disagree.  Returns the measures of the rest."""
    want = ref["radiance"]
    err = np.abs(got.astype(np.float64) - want).max(axis=-1)
    scale = np.maximum(np.abs(want).max(axis=-1), EXCLUDE_ABS)
    hit = ref["hit"]
    keep = hit & (err <= EXCLUDE_REL * scale)
    outside = float(np.abs(got[~hit]).sum())  # (a miss has no light term)
    den = float(np.abs(want[keep]).sum())
    return {"hit": int(hit.sum()), "kept": int(keep.sum()), "excluded_share": float(1.0 - keep.sum() / hit.sum()),
            "kept_sphere": int((keep & ref["sphere"]).sum()), "kept_shadowed": int((keep & ref["shadowed"]).sum()),
            "rel_l1": float(np.abs(got[keep].astype(np.float64) - want[keep]).sum() / max(den, 1e-300)),
            "light_term_outside_hits": outside}


def check_ref_case(m, bound, what):
    """The assertions every float64 case makes, on against_ref's measures."""
    assert m["light_term_outside_hits"] == 0.0, (what, m)
    assert m["excluded_share"] <= MAX_EXCLUDED, (what, m)
    assert m["kept"] >= 3500 and m["kept_sphere"] >= 400 and m["kept_shadowed"] >= 150, (what, m)
    assert m["rel_l1"] <= bound, (what, m, bound)


# ---- the threshold scene: test_gpu_lds_shading.py's floor, quads and spheres, geometry k -> material k ----------
QUADS = [(-3.5, -1.5, 0.0, 2.5, -2.0), (-1.0, 1.0, 0.5, 3.0, -3.0), (1.5, 3.5, 0.0, 2.5, -2.0)]
SPHERES = [(-2.0, 0.8, 1.0, 0.8), (0.0, 1.0, 0.5, 1.0), (2.2, 0.6, 1.5, 0.6)]


def threshold_scene():
    pos = [np.array([[-8, 0, -8], [8, 0, -8], [8, 0, 6], [-8, 0, 6]], np.float32)]
    idx = [np.array([[0, 2, 1], [0, 3, 2]], np.uint32)]
    for k, (x0, x1, y0, y1, z) in enumerate(QUADS):
        pos.append(np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32))
        idx.append(np.array([[0, 1, 2], [0, 2, 3]], np.uint32) + 4 * (k + 1))
    return {"positions": np.concatenate(pos), "indices": np.concatenate(idx),
            "tri_geom_first": np.arange(0, 10, 2, dtype=np.uint32),
            "spheres": np.array(SPHERES, np.float32), "geom_material": np.arange(7, dtype=np.uint32)}


def threshold_materials():
    """Materials on continue_path's branch edges: metallic > 0.5 is a mirror, metallic < 0.1 and ior > 1.3 is glass,
    and a diffuse path survives the roulette with probability max(albedo)."""
    f = np.float32
    return np.stack([
        mat_row(albedo=(0.5, 0.5, 0.5), roughness=0.9),                      # 0 floor: grey
        mat_row(albedo=(0.9, 0.7, 0.3), metallic=0.5, roughness=0.3),         # 1: exactly 0.5, not a mirror
        mat_row(albedo=(0.3, 0.8, 0.5), metallic=f(0.1), ior=1.5),            # 2: float32(0.1), not glass
        mat_row(albedo=(0.4, 0.5, 0.9), ior=f(1.3)),                          # 3: float32(1.3), not glass
        mat_row(albedo=(1.0, 1.0, 1.0), roughness=0.0, ior=2.4, type=1),      # 4: glass, transparency clamped at 0.95
        mat_row(albedo=(0.9, 0.8, 0.7), metallic=0.51, roughness=0.02),       # 5: just a mirror
        mat_row(albedo=(0.0, 0.0, 0.0), emission=(0.5, 2.0, 1.0)),            # 6: black emitter, surv = 0
    ])


# ---- measures -----------------------------------------------------------------------------------------------
def rel_l1(a, b):
    """Relative L1 of a against b over the entries finite on both sides."""
    m = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a[m].astype(np.float64) - b[m]).sum() / max(1e-12, np.abs(b[m].astype(np.float64)).sum()))
