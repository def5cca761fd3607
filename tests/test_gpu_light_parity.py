"""Shading parity beyond the preset state: point lights, 0 / 1 / 2 / 3 / 8 lights in either order, materials on
continue_path's branch edges and the other two integrators, each against the CPU oracle; and the direct-light term
of a depth-1 path against the float64 closed form of tests/light_ref.py.

Every frame is seen from (0, 2.2, 4.5), where geometry fills 41-76 % of the pixels.  Three measures per (scene, light
set): (a) the image under the suite's bounds (0.999 of the RGB8 pixels equal, relative L1 1e-3, the non-finite
rule); (b) the light term D = acc(set) - acc(no lights), which lights alone decide because they never steer a path,
over the pixels the oracle lights, under the same 1e-3 and exactly zero elsewhere; (c) the ray counts.  Each
(scene, set) is rendered by every launch path its light count selects (fused and separate bounces, tail depths,
one stream / side stream / shadow carry, captured graphs, straggler hand-off); those renders must agree bit for bit,
and one of them is compared with the oracle.  Nothing here is calibrated on the GPU's own output: the float64 bound
is 4 x the oracle's own error against the same reference (test_light_ref_cpu.py), not below 16 float32 epsilons.

Measures are printed, and written as profiles/light_parity_*.json under SPTR_PARITY_LOG."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library, as tests/conftest.py's renderer fixture does

import light_common as LC
import light_ref
import oracle
import residue
import sptr

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = LC.W, LC.H, 4, 6
RW, RH = 150, 82             # ragged 32x32 tiles on both edges
BW, BH, BSPP = 1000, 1010, 21  # test_gpu_bounce_order.py's batch just above 5 << 22 paths: k_shade_trace runs
ONE = ("SUN", "POINT")
MANY = ("NONE", "SUN+POINT", "POINT+SUN", "THREE", "EIGHT")
RECORDS = {}


# ---- state -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def clean(renderer):
    """The session's context with every setting these tests touch back at its default afterwards."""
    yield renderer
    renderer.set_wave_paths(0)
    renderer.set_tail_depth(0)
    renderer.set_launch_mode(0)
    renderer.set_pixel_lanes(0)
    renderer.set_stragglers(12)
    renderer.set_bvh_width(0)
    renderer.set_environment(None)
    renderer.set_materials(sptr.preset_materials(False))
    renderer.set_lights(sptr.default_lights())


@pytest.fixture(scope="module", autouse=True)
def _records():
    yield
    for group, rec in RECORDS.items():
        residue.log_parity(f"light_parity_{group}", rec)


def _record(group, case, rec):
    print(group, case, rec)
    RECORDS.setdefault(group, {})[case] = rec


def _light(row):
    return sptr.Light(int(row[0]), (C.c_float * 3)(*row[1:4]), (C.c_float * 3)(*row[4:7]), float(row[7]))


def lights_of(name):
    """The set as sptr.Light structs; the oracle takes the same rows through sptr.lights_as_array."""
    sun = sptr.default_lights()
    assert np.array_equal(sptr.lights_as_array(sun), LC.light_rows("SUN"))
    return [sun[0] if row is LC.SUN else _light(row) for row in LC.LIGHT_SETS[name]]


def _materials(rows):
    out = []
    for r in np.asarray(rows, np.float32).reshape(-1, 12):
        m = sptr.Material()
        m.albedo[:] = [float(x) for x in r[0:3]]
        m.metallic, m.roughness, m.ior, m.type = float(r[3]), float(r[4]), float(r[8]), int(r[9])
        m.emission[:] = [float(x) for x in r[5:8]]
        out.append(m)
    assert np.array_equal(sptr.materials_as_array(out).view(np.uint32), np.asarray(rows, np.float32).reshape(-1, 12).view(np.uint32))
    return out


def _flat(d):
    return sptr.FlatScene(positions=d["positions"], indices=d["indices"], tri_geom_first=d["tri_geom_first"],
                          spheres=d["spheres"], geom_material=d["geom_material"])


_ORACLE = {}


def _scene(name):
    """(FlatScene for the GPU, oracle.Prepared, materials, their rows) of a scene class, prepared once."""
    if name not in _ORACLE:
        if name == "emitter":
            flat, prep, mats = sptr.builtin_scene("default_emitter"), oracle.builtin_scene("default_emitter"), sptr.preset_materials(True)
        elif name == "threshold":
            flat, prep, mats = _flat(LC.threshold_scene()), LC.threshold_scene(), _materials(LC.threshold_materials())
        elif name == "ref":
            flat, prep, mats = _flat(LC.ref_scene()), LC.ref_scene(), None
        else:
            n = (40, 80) if name == "mesh" else (300, 600)
            flat, prep, mats = sptr.builtin_scene("sphere_mesh", *n), oracle.builtin_scene("sphere_mesh", *n), sptr.preset_materials(False)
        _ORACLE[name] = (flat, oracle.Prepared(prep, bvh=True), mats, None if mats is None else sptr.materials_as_array(mats))
    return _ORACLE[name]


def _setup(r, name):
    flat, _, mats, _ = _scene(name)
    r.set_bvh_width(0)
    r.upload_scene(flat)
    if mats is not None:
        r.set_materials(mats)
    r.set_environment(None)
    lay = r.scene_layout()
    if name in ("emitter", "threshold", "ref"):
        assert lay["lds_bytes"] != 0, lay
    else:
        assert lay["lds_bytes"] == 0 and lay["bvh_width"] == 4, lay


def _cam(w, h, target=LC.CAM_TARGET):
    return sptr.camera_lookat(LC.CAM_POS, target, aspect=w / h)


_OCACHE = {}


def _oracle(name, lset, w=W, h=H, spp=SPP, depth=DEPTH, target=LC.CAM_TARGET, mats=None, **kw):
    """The oracle's (accum, rgb8, counters) of a frame; computed once per distinct frame and left unchanged."""
    lkey = lset if isinstance(lset, str) else np.asarray(lset, np.float32).tobytes()
    key = (name, lkey, w, h, spp, depth, target, None if mats is None else mats.tobytes(),
           tuple((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(kw.items())))
    if key not in _OCACHE:
        _, P, _, rows = _scene(name)
        lts = sptr.lights_as_array(lights_of(lset)) if isinstance(lset, str) else np.asarray(lset, np.float32).reshape(-1, 8)
        _OCACHE[key] = P.render(_cam(w, h, target).as_array(), w, h, rows if mats is None else mats, lts, frames=spp,
                                max_depth=depth, threads=LC.THREADS, **kw)
    return _OCACHE[key]


class Shot:
    def __init__(self, r, st):
        self.acc, self.rgb = r.read_accum().copy(), r.read_rgb8().copy()
        self.closest, self.shadow, self.fused, self.handed = int(st.rays_closest), int(st.rays_shadow), int(st.traced_fused), int(st.paths_handed_off)


def _shoot(r, cam, w=W, h=H, spp=SPP, depth=DEPTH, flags=0, tail=0, mode=0, calls=1, stragglers=None, **kw):
    """`calls` renders of one frame with the given tail depth, launch mode and flags; all must be the same."""
    r.set_tail_depth(tail)
    r.set_launch_mode(mode)
    if stragglers is not None:
        r.set_stragglers(stragglers)
    try:
        shots = [Shot(r, r.render(cam, w, h, spp=spp, max_depth=depth, flags=flags, **kw)) for _ in range(calls)]
        if mode == 3 and calls > 1 and not kw:
            assert r.graph_info()["valid"] == 1  # (the second call captured, the third replayed)
    finally:
        r.set_tail_depth(0)
        r.set_launch_mode(0)
        if stragglers is not None:
            r.set_stragglers(12)
    for s in shots[1:]:
        _same(shots[0], s, ("repeat", tail, mode, flags))
    return shots[0]


def _same(a, b, what):
    assert np.array_equal(a.acc.view(np.uint32), b.acc.view(np.uint32)), (what, "accum")
    assert np.array_equal(a.rgb, b.rgb), (what, "rgb8")
    assert (a.closest, a.shadow) == (b.closest, b.shadow), (what, "counts", a.closest, a.shadow, b.closest, b.shadow)


def _variants(r, cam, variants, what, **kw):
    """Render every variant (a dict of _shoot's arguments); all bit-identical; returns them in order."""
    shots = [_shoot(r, cam, **kw, **v) for v in variants]
    for v, s in zip(variants[1:], shots[1:]):
        _same(shots[0], s, (what, v))
    return shots


# ---- the comparison with the oracle -----------------------------------------------------------------------------
def _image_close(rgb, orgb, acc, oacc, exact_frac=0.999, rel_l1=1e-3):
    """test_gpu_parity.py's bounds; returns the measures, the caller asserts after printing them."""
    frac = float((rgb == orgb).all(axis=2).mean())
    fin, ofin = np.isfinite(acc), np.isfinite(oacc)
    return {"exact": frac, "rel_l1": LC.rel_l1(acc, oacc), "nonfinite_differ": int((fin != ofin).sum()),
            "ok": bool(frac >= exact_frac and LC.rel_l1(acc, oacc) <= rel_l1 and (fin != ofin).sum() <= max(3, 1e-6 * fin.size))}


def _light_term(lit, dark, olit, odark, pixels=None):
    """(b): D against the oracle's over the pixels it lights; D == 0 bit for bit where the oracle's is 0 and the
    two no-light images agree.  Arrays (..., 3); pixels: a mask of the pixels compared (default all)."""
    D, Do = lit - dark, olit - odark
    on = (Do != 0).any(axis=-1)
    same_dark = (dark.view(np.uint32) == odark.view(np.uint32)).all(axis=-1)
    off = ~on & same_dark
    if pixels is not None:
        on, off = on & pixels, off & pixels
    n = int(pixels.sum()) if pixels is not None else on.size
    return {"lit_share": float(on.sum() / n), "rel_l1_lit": LC.rel_l1(D[on], Do[on]) if on.any() else 0.0,
            "unlit_compared": int(off.sum()), "unlit_nonzero": int((D[off].view(np.uint32) != 0).any(axis=-1).sum())}


def _against_oracle(group, case, name, lset, shot, dark, want, odark, min_lit=None, exact=0.999, rel=1e-3, count_rel=1e-3):
    oacc, orgb, ocnt = want
    rec = {"image": _image_close(shot.rgb, orgb, shot.acc, oacc, exact, rel),
           "rays": {"closest": shot.closest, "shadow": shot.shadow, "oracle_closest": ocnt["rays_closest"], "oracle_shadow": ocnt["rays_shadow"]}}
    if lset != "NONE":
        rec["light_term"] = _light_term(shot.acc, dark.acc, oacc, odark[0])
    _record(group, case, rec)
    assert rec["image"]["ok"], rec
    assert shot.closest == dark.closest and dark.shadow == 0, rec                 # (c): lights never steer a path
    assert abs(shot.shadow - ocnt["rays_shadow"]) <= count_rel * ocnt["rays_shadow"] + 5, rec
    if lset == "NONE":
        assert shot.shadow == 0 and ocnt["rays_shadow"] == 0
        return rec
    lt = rec["light_term"]
    assert lt["rel_l1_lit"] <= rel, rec
    assert lt["unlit_nonzero"] == 0 and lt["unlit_compared"] > 0, rec
    if min_lit is not None:
        assert lt["lit_share"] >= min_lit, rec
    return rec


def _dark(r, name, cam, **kw):
    r.set_lights([])
    return _shoot(r, cam, **kw)


MODE3 = dict(mode=3, calls=3)


# ---- 1. LDS-staged scenes -----------------------------------------------------------------------------------------
def test_threshold_scene_is_in_view():
    """Every geometry of the threshold scene is the first hit of >= 150 pixels (measured 170-2369)."""
    _, P, _, _ = _scene("threshold")
    cam = _cam(W, H).as_array()
    d, _ = oracle.primary(cam, W, H, 1)
    rays = np.zeros((W * H, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = cam[:3], d.reshape(-1, 3), np.inf
    g = P.intersect(rays)[0]
    counts = [int((g == k).sum()) for k in range(7)]
    _record("scenes", "threshold_first_hits", {"per_geometry": counts, "hit_share": float((g != 0xFFFFFFFF).mean())})
    assert min(counts) >= 150, counts


@pytest.mark.parametrize("lset", ONE)
@pytest.mark.parametrize("name", ["emitter", "threshold"])
def test_lds_one_light(clean, name, lset):
    """One light fuses the shadow ray into the bounce kernels: the default call, the separate k_trace / k_shade /
    k_shadow (COUNT_VISITS), k_tail from depth 1, from depth 3 and never, and a captured graph with its replay."""
    r, cam = clean, _cam(W, H)
    _setup(r, name)
    dark = _dark(r, name, cam)
    r.set_lights(lights_of(lset))
    shots = _variants(r, cam, [dict(), dict(flags=sptr.SPTR_FRAME_COUNT_VISITS), dict(tail=1), dict(tail=3), dict(tail=32), MODE3],
                      (name, lset))
    assert shots[0].fused > 0 and shots[1].fused == 0
    _against_oracle("lds", f"{name}_{lset}", name, lset, shots[0], dark, _oracle(name, lset), _oracle(name, "NONE"),
                    min_lit=0.25 if name == "emitter" else None)


@pytest.mark.parametrize("lset", MANY)
@pytest.mark.parametrize("name", ["emitter", "threshold"])
def test_lds_many_lights(clean, name, lset):
    """No light, or several: the shadow tasks go through the task stream (two float4 each, three with a point
    light) and k_shadow; nothing fuses."""
    r, cam = clean, _cam(W, H)
    _setup(r, name)
    dark = _dark(r, name, cam)
    r.set_lights(lights_of(lset))
    shots = _variants(r, cam, [dict(), dict(tail=2), dict(tail=32), MODE3], (name, lset))
    assert shots[0].fused == 0
    if lset == "NONE":
        _same(shots[0], dark, "two renders without lights")
    _against_oracle("lds", f"{name}_{lset}", name, lset, shots[0], dark, _oracle(name, lset), _oracle(name, "NONE"),
                    min_lit=0.25 if name == "emitter" else None)


@pytest.mark.parametrize("name", ["emitter", "threshold", "mesh"])
def test_light_order(clean, name):
    """(d) SUN+POINT against POINT+SUN: the order of two float32 additions per path vertex (the oracle: 2.7e-9)."""
    r, cam = clean, _cam(W, H)
    _setup(r, name)
    r.set_lights(lights_of("SUN+POINT"))
    a = _shoot(r, cam)
    r.set_lights(lights_of("POINT+SUN"))
    b = _shoot(r, cam)
    rel = LC.rel_l1(b.acc, a.acc)
    _record("order", name, {"rel_l1": rel, "oracle_rel_l1": LC.rel_l1(_oracle(name, "POINT+SUN")[0], _oracle(name, "SUN+POINT")[0])})
    assert (a.closest, a.shadow) == (b.closest, b.shadow)
    assert rel <= 1e-6, rel


@pytest.mark.parametrize("name,lset", [("emitter", "EIGHT"), ("threshold", "POINT"), ("mesh", "THREE"), ("bigmesh", "SUN+POINT")])
def test_ragged_tiles(clean, name, lset):
    """150 x 82: tile slots outside the image on both edges, several blocks."""
    r, cam = clean, _cam(RW, RH)
    _setup(r, name)
    kw = dict(w=RW, h=RH)
    dark = _dark(r, name, cam, **kw)
    r.set_lights(lights_of(lset))
    shots = _variants(r, cam, [dict(), dict(flags=sptr.SPTR_FRAME_COUNT_VISITS), MODE3], (name, lset, "ragged"), **kw)
    _against_oracle("ragged", f"{name}_{lset}", name, lset, shots[0], dark, _oracle(name, lset, **kw), _oracle(name, "NONE", **kw))


@pytest.mark.parametrize("name", ["emitter", "threshold"])
def test_big_batch_point_light(clean, name):
    """One batch of 1000 x 1010 x 21 paths, where k_shade_trace runs the fused bounces, with the point light:
    against its separate-launch twin bit for bit, and against the oracle at 4096 sampled pixels."""
    r, cam = clean, _cam(BW, BH)
    _setup(r, name)
    r.set_pixel_lanes(1)
    kw = dict(w=BW, h=BH, spp=BSPP)
    dark = _dark(r, name, cam, **kw)
    r.set_lights(lights_of("POINT"))
    shots = _variants(r, cam, [dict(), dict(flags=sptr.SPTR_FRAME_COUNT_VISITS)], (name, "big batch"), **kw)
    assert shots[0].fused > 0 and shots[1].fused == 0
    assert shots[0].closest == dark.closest and dark.shadow == 0
    pix = np.sort(np.random.default_rng(1).choice(BW * BH, 4096, replace=False)).astype(np.uint32)
    mask = np.zeros(BW * BH, bool)
    mask[pix] = True
    mask = mask.reshape(BH, BW)
    oacc = _oracle(name, "POINT", **kw, pixels=pix)[0]
    odark = _oracle(name, "NONE", **kw, pixels=pix)[0]
    lt = _light_term(shots[0].acc, dark.acc, oacc, odark, pixels=mask)
    rec = {"rel_l1": LC.rel_l1(shots[0].acc[mask], oacc[mask]), "rel_l1_dark": LC.rel_l1(dark.acc[mask], odark[mask]),
           "nonfinite_differ": int((np.isfinite(shots[0].acc[mask]) != np.isfinite(oacc[mask])).sum()), "light_term": lt}
    _record("big_batch", name, rec)
    assert rec["rel_l1"] <= 1e-3 and rec["rel_l1_dark"] <= 1e-3 and rec["nonfinite_differ"] <= 3, rec
    assert lt["rel_l1_lit"] <= 1e-3 and lt["unlit_nonzero"] == 0 and lt["unlit_compared"] > 0, rec
    if name == "emitter":
        assert lt["lit_share"] >= 0.25, rec


# ---- 2. the mesh in L2, and the one beyond an XCD's L2 -------------------------------------------------------------
@pytest.mark.parametrize("lset", ONE)
def test_l2_mesh_one_light(clean, lset):
    """sphere_mesh 40 x 80, a BVH4 walked from L2: one stream (mode 2), the side stream with k_shadow_dyn (1), the
    shadow carry into k_tail (0), a captured graph (3); tail depths 2 and 32 in mode 0."""
    r, cam = clean, _cam(W, H)
    _setup(r, "mesh")
    dark = _dark(r, "mesh", cam)
    r.set_lights(lights_of(lset))
    shots = _variants(r, cam, [dict(mode=2), dict(mode=1), dict(mode=0), MODE3, dict(tail=2), dict(tail=32)], ("mesh", lset))
    _against_oracle("mesh", lset, "mesh", lset, shots[0], dark, _oracle("mesh", lset), _oracle("mesh", "NONE"), min_lit=0.25)


@pytest.mark.parametrize("lset", MANY)
def test_l2_mesh_many_lights(clean, lset):
    r, cam = clean, _cam(W, H)
    _setup(r, "mesh")
    dark = _dark(r, "mesh", cam)
    r.set_lights(lights_of(lset))
    shots = _variants(r, cam, [dict(mode=2), dict(mode=0)] + ([dict(tail=32)] if lset == "EIGHT" else []), ("mesh", lset))
    if lset == "NONE":
        _same(shots[0], dark, "two renders without lights")
    _against_oracle("mesh", lset, "mesh", lset, shots[0], dark, _oracle("mesh", lset), _oracle("mesh", "NONE"), min_lit=0.25)


@pytest.mark.parametrize("lset", ["THREE", "POINT"])
def test_big_mesh_stragglers(clean, lset):
    """sphere_mesh 300 x 600 (360 K triangles, beyond one XCD's L2), 128 x 96 x 8: no hand-off and every drained
    wave's rays handed to k_strag."""
    r, w, h, spp = clean, 128, 96, 8
    cam = _cam(w, h)
    _setup(r, "bigmesh")
    kw = dict(w=w, h=h, spp=spp)
    dark = _dark(r, "bigmesh", cam, stragglers=0, **kw)
    r.set_lights(lights_of(lset))
    shots = _variants(r, cam, [dict(stragglers=0), dict(stragglers=64)], ("bigmesh", lset), **kw)
    assert shots[0].handed == 0
    if lset == "POINT":
        assert shots[1].handed > 0
    _against_oracle("bigmesh", lset, "bigmesh", lset, shots[0], dark, _oracle("bigmesh", lset, **kw), _oracle("bigmesh", "NONE", **kw))


# ---- 3. the other two integrators ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lset", ["NONE", "SUN+POINT", "EIGHT"])
@pytest.mark.parametrize("integ", ["pathtracer", "optix"])
def test_integrators(clean, integ, lset):
    """k_pathtracer's light loop and k_optix on default_emitter under test_pathtracer.py's and test_optix_mode.py's
    bounds (0.995 of the pixels, 2e-3 relative L1) and count rules."""
    r, cam = clean, _cam(W, H)
    _setup(r, "emitter")
    r.set_lights(lights_of(lset))
    if integ == "pathtracer":
        s = _shoot(r, cam, integrator=sptr.SPTR_INTEGRATOR_PATHTRACER, samples_per_frame=4)
        oacc, orgb, ocnt = _oracle("emitter", lset, pathtracer_spf=4)
    else:
        s = _shoot(r, cam, integrator=sptr.SPTR_INTEGRATOR_OPTIX)
        oacc, orgb, ocnt = _oracle("emitter", lset, optix=True)
    rec = {"image": _image_close(s.rgb, orgb, s.acc, oacc, 0.995, 2e-3),
           "rays": {"closest": s.closest, "shadow": s.shadow, "oracle_closest": ocnt["rays_closest"], "oracle_shadow": ocnt["rays_shadow"]}}
    _record("integrators", f"{integ}_{lset}", rec)
    assert rec["image"]["ok"] and rec["image"]["nonfinite_differ"] == 0, rec
    assert abs(s.closest - ocnt["rays_closest"]) <= 2e-3 * ocnt["rays_closest"], rec
    if integ == "optix" or lset == "NONE":
        assert s.shadow == 0 and ocnt["rays_shadow"] == 0, rec
    else:
        assert ocnt["rays_shadow"] > 0 and abs(s.shadow - ocnt["rays_shadow"]) <= 2e-3 * ocnt["rays_shadow"] + 5, rec


# ---- 4. float64 ---------------------------------------------------------------------------------------------------
def _float64_case(r, mat, light, lights, case):
    row = LC.REF_MATS[mat]
    rows = np.stack([row, row])
    cam = _cam(W, H, LC.CAM_TARGET_REF)
    dirs, _ = oracle.primary(cam.as_array(), W, H, 1)
    ref = light_ref.direct_light(cam.as_array()[:3], dirs, row, row, LC.REF_LIGHTS[light])
    kw = dict(spp=1, depth=1, target=LC.CAM_TARGET_REF, mats=rows)
    o = LC.against_ref(_oracle("ref", [LC.REF_LIGHTS[light]], **kw)[0] - _oracle("ref", [], **kw)[0], ref)
    _setup(r, "ref")
    r.set_materials(_materials(rows))
    r.set_lights([])
    dark = _shoot(r, cam, spp=1, depth=1)
    r.set_lights([_light(x) for x in lights])
    lit = _shoot(r, cam, spp=1, depth=1)
    m = LC.against_ref(lit.acc - dark.acc, ref)
    bound = max(4.0 * o["rel_l1"], LC.FLOOR_EPS)
    _record("float64", case, {"gpu": m, "d_case": o["rel_l1"], "oracle_excluded_share": o["excluded_share"], "bound": bound})
    assert lit.closest == dark.closest == W * H and dark.shadow == 0
    LC.check_ref_case(m, bound, case)
    return lit


@pytest.mark.parametrize("light", list(LC.REF_LIGHTS))
@pytest.mark.parametrize("mat", list(LC.REF_MATS))
def test_light_term_against_float64(clean, mat, light):
    """The GPU's acc(light) - acc(no light) of a depth-1, 1-spp frame of light_ref's scene against the float64
    closed form: at most 0.5 % of the hit pixels excluded, relative L1 over the rest within max(4 d_case, 16 eps),
    d_case being the oracle's relative L1 against the same reference, computed here.  One light on a staged scene:
    k_shade traces the shadow ray in place."""
    _float64_case(clean, mat, light, [LC.REF_LIGHTS[light]], f"{mat}_{light}")


def test_light_term_against_float64_through_the_task_stream(clean):
    """POINT behind a FILL of intensity 0: two lights, so the shadow tasks go through the stream and k_shadow reads
    the point light's direction from the task's third float4; the dark light adds exactly nothing."""
    fill0 = list(LC.FILL[:7]) + [0.0]
    _float64_case(clean, "m0.4_r0.3_ior1.2", "POINT", [fill0, LC.POINT], "m0.4_r0.3_ior1.2_FILL0+POINT")


# ---- 5. transitions on one context --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["emitter", "mesh"])
def test_light_set_transitions(name):
    """SUN -> EIGHT -> NONE -> POINT -> THREE -> SUN on one fresh context in launch mode 3, three calls each: the task
    stream grows, the task stride goes 2 -> 3 -> 2 and every change invalidates the captured graph.  Each set's
    image equals, bit for bit, the one of a context that has only ever had that set."""
    seq = ["SUN", "EIGHT", "NONE", "POINT", "THREE", "SUN"]
    cam = _cam(W, H)

    def fresh():
        r = sptr.Renderer(0)
        _setup(r, name)
        return r

    want = {}
    for lset in sorted(set(seq)):
        r = fresh()
        try:
            r.set_lights(lights_of(lset))
            want[lset] = _shoot(r, cam, **MODE3)
        finally:
            r.close()
    r = fresh()
    try:
        for lset in seq:
            r.set_lights(lights_of(lset))
            _same(want[lset], _shoot(r, cam, **MODE3), (name, "after the sets before", lset))
    finally:
        r.close()
