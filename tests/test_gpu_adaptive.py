"""GPU tests of adaptive sampling: sptr_render_adaptive / sptr_read_sample_counts (kernels_adaptive.h: the
selection, k_adapt_inject, k_adapt_gather, k_adapt_resolve, and the chain of the ray path between them) through
Renderer.render_adaptive / read_sample_counts and sptr_cli --adaptive.

The yardsticks are the renderer's own frames and tests/adaptive_ref.py: sample i of a pixel is what frame i of
sptr_render takes there, so L[i] comes from single-sample render calls under seed offset i - 1, the numpy float32
restatement of the rule turns L into (S, E, n, passes), and the device must return exactly that.  "Equal" is
equality of the uint32 bit patterns.  Nothing here has a tolerance."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as tests/conftest.py's renderer fixture does)

import adaptive_ref as AR
import residue
import sptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W, H = 96, 64
CASE2 = dict(threshold=0.02, min_samples=8, max_samples=32, step=4)
SHAPE = dict(threshold=0.02, min_samples=2, max_samples=7, step=3)  # takes 2, 3, 2: the last one is cut


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _equal(got, want, what):
    got, want = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    print(f"{what}: {bad} of {got.size} words differ")
    assert bad == 0, what


def _rc(call):
    """The return code of a call that must fail."""
    with pytest.raises(sptr.SptrError) as e:
        call()
    return int(str(e.value).split("rc=")[1].split(":")[0])


@pytest.fixture()
def clean(renderer):
    yield renderer
    renderer.set_wave_paths(0)
    renderer.set_seed_offset(0)
    renderer.set_denoise(0)
    renderer.set_bvh_width(0)
    renderer.set_lights(sptr.default_lights())


def _emitter(r):
    r.set_bvh_width(0)
    sptr.setup_default(r, "default_emitter")
    assert r.scene_layout()["lds_bytes"] != 0


def _cam2(w=W, h=H):
    return sptr.camera_lookat(pos=(0.0, 2.0, 5.0), target=(0.0, 1.0, 0.0), fov=45.0, aspect=w / h)


def _samples(r, cam, w, h, n, depth):
    """L[i - 1] (w * h, 3): sample i of every pixel, from single-sample frames under seed offset i - 1."""
    L = np.empty((n, w * h, 3), np.float32)
    try:
        for i in range(1, n + 1):
            r.set_seed_offset(i - 1)
            r.render(cam, w, h, spp=1, max_depth=depth)
            L[i - 1] = r.read_accum().reshape(-1, 3)
    finally:
        r.set_seed_offset(0)
    return L


_REF = {}


def _reference(r, w, h, params, depth=6):
    """adaptive_ref's (S, E, n, passes) and L for the emitter scene at w x h under params, computed once."""
    key = (w, h, depth, tuple(sorted(params.items())))
    _emitter(r)
    if key not in _REF:
        L = _samples(r, _cam2(w, h), w, h, params["max_samples"], depth)
        L.setflags(write=False)
        out = AR.run(L, **params)
        for a in out[:3]:
            a.setflags(write=False)
        _REF[key] = (L,) + out
    return _REF[key]


def _check_against(r, info, ref, w, h, what, rgb=True):
    L, S, E, n, passes = ref
    cnt = r.read_sample_counts()
    assert cnt.shape == (h, w) and cnt.dtype == np.uint32
    bad = int((cnt.reshape(-1) != n).sum())
    print(f"{what}: {bad} of {n.size} counts differ; passes {info['passes']} (reference {passes}), "
          f"samples {info['samples']}, chunks {info['chunks']}, {info['ms']:.2f} ms")
    assert bad == 0, what
    _equal(r.read_accum().reshape(-1, 3), S, what + ": S")
    if rgb:
        want = residue.resolve_device_gamma(r, S, n.astype(np.float32)[:, None])
        assert np.array_equal(r.read_rgb8().reshape(-1, 3), want), what + ": RGB8"
    assert info["samples"] == int(n.sum()) and info["passes"] == passes
    assert info["min_count"] == int(n.min()) and info["max_count"] == int(n.max())
    assert info["rays_closest"] >= info["samples"] and info["ms"] > 0.0


# ------------------------------------------------------------------------------- 1. threshold 0 is the frame path
@pytest.mark.parametrize("depth", [1, 6])
@pytest.mark.parametrize("scene", ["default_emitter", "mesh"])
def test_threshold_zero_equals_the_frame_path(clean, scene, depth):
    r = clean
    r.set_bvh_width(0)
    if scene == "mesh":  # too large to be staged: walked as BVH4
        sptr.setup_default(r, "sphere_mesh", 40, 80)
        lay = r.scene_layout()
        assert lay["lds_bytes"] == 0 and lay["bvh_width"] == 4
    else:
        _emitter(r)
    cam = sptr.camera_lookat(aspect=W / H)
    r.render(cam, W, H, spp=8, max_depth=depth)
    acc, rgb = r.read_accum(), r.read_rgb8()
    info = r.render_adaptive(cam, W, H, 0.0, 4, 8, 2, max_depth=depth)
    _equal(r.read_accum(), acc, f"{scene} depth {depth}: S vs sptr_render(spp=8)")
    assert np.array_equal(r.read_rgb8(), rgb)
    assert (r.read_sample_counts() == 8).all()
    assert info["samples"] == 8 * W * H and info["passes"] == 3 and (info["min_count"], info["max_count"]) == (8, 8)
    assert info["active_first"] == W * H and info["active_last"] == W * H


# ------------------------------------------------------------------------------- 2. the rule against the reference
def test_rule_against_the_reference(clean):
    r = clean
    ref = _reference(r, W, H, CASE2)
    n = ref[3]
    at_min, between, at_max = (float((n == 8).mean()), float(((n > 8) & (n < 32)).mean()),
                               float(((n == 32) & AR.active(ref[1], ref[2], n, 0.02, 8, 33)).mean()))
    print(f"reference counts: {at_min:.3f} stop at 8, {between:.3f} in between, {at_max:.3f} reach 32 unconverged")
    assert at_min >= 0.10 and between >= 0.10 and at_max >= 0.10  # (the rule is exercised: the test is not vacuous)
    info = r.render_adaptive(_cam2(), W, H, max_depth=6, **CASE2)
    _check_against(r, info, ref, W, H, "case 2")
    assert info["active_first"] == W * H and 0 < info["active_last"] < W * H


# ------------------------------------------------------------------------------- 3. shapes where indexing can break
@pytest.mark.parametrize("w,h", [(1, 1), (33, 31), (64, 32), (150, 82)])
def test_shapes(clean, w, h):
    r = clean
    ref = _reference(r, w, h, SHAPE)
    info = r.render_adaptive(_cam2(w, h), w, h, max_depth=6, **SHAPE)
    _check_against(r, info, ref, w, h, f"{w} x {h}")


# ------------------------------------------------------------------------------- 4. chunks cannot matter
@pytest.mark.parametrize("wave_paths", [16384, 3])
def test_chunks_cannot_matter(clean, wave_paths):
    """16384: the first pass (6144 pixels x 8 samples) takes three chunks.  3: below step = 4, so every entry's
    take is split over chunks.  A guard word around E, n or the list that changed makes the call SPTR_ERR_HIP."""
    r = clean
    ref = _reference(r, W, H, CASE2)
    one = r.render_adaptive(_cam2(), W, H, max_depth=6, **CASE2)
    r.set_wave_paths(wave_paths)  # (a setting: the state epoch moves, the next call starts anew anyway)
    info = r.render_adaptive(_cam2(), W, H, max_depth=6, **CASE2)
    _check_against(r, info, ref, W, H, f"wave_paths {wave_paths}")
    assert info["chunks"] >= one["chunks"] + 2
    if wave_paths < CASE2["step"]:
        assert info["chunks"] >= info["samples"] // wave_paths
    assert (info["rays_closest"], info["rays_shadow"]) == (one["rays_closest"], one["rays_shadow"])


# ------------------------------------------------------------------------------- 5. continue
def test_continue_equals_one_call(clean):
    r = clean
    ref = _reference(r, W, H, CASE2)
    cam = _cam2()
    first = r.render_adaptive(cam, W, H, 0.02, 8, 16, 4, max_depth=6)
    assert first["max_count"] == 16
    second = r.render_adaptive(cam, W, H, max_depth=6, cont=True, **CASE2)
    L, S, E, n, passes = ref
    assert first["samples"] + second["samples"] == int(n.sum()) and first["passes"] + second["passes"] == passes
    assert (r.read_sample_counts().reshape(-1) == n).all()
    _equal(r.read_accum().reshape(-1, 3), S, "max 16 continued to max 32: S")
    assert np.array_equal(r.read_rgb8().reshape(-1, 3), residue.resolve_device_gamma(r, S, n.astype(np.float32)[:, None]))
    # a continuation with nothing left to do
    idle = r.render_adaptive(cam, W, H, max_depth=6, cont=True, **CASE2)
    assert idle["samples"] == 0 and idle["passes"] == 0 and idle["chunks"] == 0 and idle["max_count"] == 32
    _equal(r.read_accum().reshape(-1, 3), S, "idle continuation: S")


def test_continue_under_other_parameters(clean):
    """A continuation whose pixels hold different counts and take different amounts in one pass (n = 8 .. 16,
    max 21, step 7: takes 7 and 5) equals the reference continued from the first call's state."""
    r = clean
    L, S, E, n, passes = _reference(r, W, H, CASE2)
    cam = _cam2()
    r.render_adaptive(cam, W, H, 0.02, 8, 16, 4, max_depth=6)
    state = AR.run(L, 0.02, 8, 16, 4)
    want = AR.run(L, 0.005, 8, 21, 7, state=state[:3])
    assert len(np.unique(AR.take(state[2], 8, 21, 7)[AR.active(*state[:3], 0.005, 8, 21)])) >= 2
    info = r.render_adaptive(cam, W, H, 0.005, 8, 21, 7, max_depth=6, cont=True)
    assert (r.read_sample_counts().reshape(-1) == want[2]).all()
    _equal(r.read_accum().reshape(-1, 3), want[0], "continued under other parameters: S")
    assert info["passes"] == want[3] and info["samples"] == int(want[2].sum()) - int(state[2].sum())


def test_continue_needs_the_same_call(clean):
    r = clean
    _emitter(r)
    cam = _cam2()
    args = dict(max_depth=6, cont=True, **CASE2)
    r.render_adaptive(cam, W, H, 0.02, 8, 16, 4, max_depth=6)
    moved = sptr.camera_lookat(pos=(0.1, 2.0, 5.0), target=(0.0, 1.0, 0.0), fov=45.0, aspect=W / H)
    assert _rc(lambda: r.render_adaptive(moved, W, H, **args)) == -1
    assert _rc(lambda: r.render_adaptive(_cam2(64, 32), 64, 32, **args)) == -1
    assert _rc(lambda: r.render_adaptive(cam, W, H, **dict(args, max_depth=5))) == -1
    assert _rc(lambda: r.render_adaptive(cam, W, H, shard=(0, 2), **args)) == -1
    r.render_adaptive(cam, W, H, **args)  # the refused calls left the state alone
    r.set_lights(sptr.default_lights())   # the state epoch moves
    assert _rc(lambda: r.render_adaptive(cam, W, H, **args)) == -1
    r.render_adaptive(cam, W, H, 0.02, 8, 16, 4, max_depth=6)
    r.render(cam, W, H, spp=1, max_depth=6)  # a render call overwrites the accumulation
    assert _rc(lambda: r.render_adaptive(cam, W, H, **args)) == -1
    assert _rc(lambda: r.read_sample_counts()) == -1


# ------------------------------------------------------------------------------- 6. shards
def test_a_shard_equals_its_pixels_of_the_whole(clean):
    r = clean
    L, S, E, n, passes = _reference(r, W, H, CASE2)
    info = r.render_adaptive(_cam2(), W, H, max_depth=6, shard=(1, 3), **CASE2)
    ys, xs = np.mgrid[0:H, 0:W]
    mine = (((ys // 32) * ((W + 31) // 32) + xs // 32) % 3 == 1).reshape(-1)
    assert 0 < mine.sum() < W * H
    cnt, acc = r.read_sample_counts().reshape(-1), r.read_accum().reshape(-1, 3)
    assert (cnt[mine] == n[mine]).all() and (cnt[~mine] == 0).all()
    _equal(acc[mine], S[mine], "rank 1 of 3: S on its pixels")
    assert not acc[~mine].any()
    assert info["samples"] == int(n[mine].sum()) and info["active_first"] == int(mine.sum())


# ------------------------------------------------------------------------------- 7. the context afterwards
def _golden(r):
    g = np.load(os.path.join(GOLD, "radiance.npz"), allow_pickle=False)
    cam = sptr.camera_lookat(aspect=64 / 48)
    st = r.render(cam, 64, 48, spp=1, max_depth=6)
    rgb, acc = r.read_rgb8(), r.read_accum()
    frac = float((rgb == g["default_emitter_d6_rgb"]).all(axis=2).mean())
    rel = float(np.abs(acc - g["default_emitter_d6_accum"]).sum() / np.abs(g["default_emitter_d6_accum"]).sum())
    assert frac >= 0.995 and rel <= 5e-3, (frac, rel)  # (tests/test_gpu_golden.py's criteria for this frame)
    return st, acc


COUNTERS = ("rays_closest", "rays_shadow", "samples", "waves", "rays_tail", "traced_primary", "traced_bounce",
            "traced_by_depth", "traced_fused", "paths_handed_off", "cull_launches")


def test_the_golden_frame_and_its_stats_after_an_adaptive_call(clean):
    r = clean
    _emitter(r)
    st0, acc0 = _golden(r)
    st1, acc1 = _golden(r)  # (a repeat without an adaptive call in between: what "the same" means)
    cam = sptr.camera_lookat(aspect=64 / 48)  # the golden frame's camera and size: its cull mask stays valid
    info = r.render_adaptive(cam, 64, 48, max_depth=6, **CASE2)
    assert info["rays_closest"] > info["samples"] > 0 and info["min_count"] < info["max_count"]
    assert _rc(lambda: r.render(cam, 64, 48, spp=1, frame_begin=info["max_count"] + 1, max_depth=6)) == -1
    assert _rc(lambda: r.render(cam, 64, 48, spp=1, frame_begin=info["min_count"] + 1, max_depth=6)) == -1
    assert _rc(lambda: r.render(cam, 64, 48, spp=1, frame_begin=2, max_depth=6)) == -1
    nores = r.render_adaptive(cam, 64, 48, max_depth=6, frame_flags=2, **CASE2)  # SPTR_FRAME_NO_RESOLVE
    assert nores["samples"] == info["samples"]
    st2, acc2 = _golden(r)
    _equal(acc1, acc0, "golden frame repeated")
    _equal(acc2, acc0, "golden frame after an adaptive call")
    for k in COUNTERS:
        a, b, c = (st.as_dict()[k] for st in (st0, st1, st2))
        assert b == c and (a == b or k == "cull_launches"), (k, a, b, c)  # (the first call computed the cull mask)


BAD = [
    ("integrator", dict(integrator=1)),
    ("frame_begin", dict(frame_begin=2)),
    ("frame flag", dict(frame_flags=1)),  # SPTR_FRAME_TIMING
    ("min below 2", dict(min_samples=1)),
    ("max below min", dict(max_samples=7)),
    ("max above 65536", dict(max_samples=65537)),
    ("step 0", dict(step=0)),
    ("negative threshold", dict(threshold=-1.0)),
    ("nan threshold", dict(threshold=float("nan"))),
    ("infinite threshold", dict(threshold=float("inf"))),
    ("reserved", dict(reserved=(0, 1, 0))),
    ("unknown flag", dict(flags=2)),
    ("depth 0", dict(max_depth=0)),
]


def test_error_cases_leave_the_golden_frame(clean):
    r = clean
    _emitter(r)
    st0, acc0 = _golden(r)
    cam = _cam2()

    def again(what):
        st, acc = _golden(r)
        _equal(acc, acc0, "golden frame after: " + what)
        for k in COUNTERS:
            assert st.as_dict()[k] == st0.as_dict()[k] or k == "cull_launches", (what, k)

    r.set_denoise(2)
    assert _rc(lambda: r.render_adaptive(cam, W, H, max_depth=6, **CASE2)) == -1
    r.set_denoise(0)
    again("denoiser on")
    for what, over in BAD:
        kw = dict(dict(max_depth=6, **CASE2), **over)
        assert _rc(lambda: r.render_adaptive(cam, W, H, **kw)) == -1, what
        again(what)


def test_no_scene():
    r = sptr.Renderer(0)
    try:
        assert _rc(lambda: r.render_adaptive(_cam2(), W, H, max_depth=6, **CASE2)) == -3
        assert _rc(lambda: r.read_sample_counts()) == -1
    finally:
        r.close()


# ------------------------------------------------------------------------------- 8. sptr_cli --adaptive
def test_cli_adaptive(tmp_path):
    exe = os.path.join(ROOT, "simple-path-tracer_amd", "sptr_cli")
    assert os.path.exists(exe), "sptr_cli not built (make -C simple-path-tracer_amd)"
    w, h = 64, 32
    out, counts = tmp_path / "a.ppm", tmp_path / "counts.pfm"
    res = subprocess.run([exe, "--scene", "default_emitter", "--w", str(w), "--h", str(h), "--adaptive", "0.02", "--min-spp", "8",
                          "--spp", "32", "--step", "4", "--depth", "6", "--json", "--out", str(out), "--counts", str(counts)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    with open(counts, "rb") as f:
        assert f.readline() == b"Pf\n" and f.readline() == b"%d %d\n" % (w, h) and f.readline() == b"-1.0\n"
        cnt = np.frombuffer(f.read(), "<f4").reshape(h, w)
    with open(out, "rb") as f:
        assert f.readline() == b"P6\n" and f.readline() == b"%d %d\n" % (w, h) and f.readline() == b"255\n"
        img = np.frombuffer(f.read(), np.uint8).reshape(h, w, 3)
    assert abs(info["adaptive"] - 0.02) < 1e-6 and (info["min_spp"], info["max_spp"], info["step"]) == (8, 32, 4)
    assert (info["width"], info["height"], info["depth"]) == (w, h, 6)
    assert (info["min_count"], info["max_count"]) == (int(cnt.min()), int(cnt.max()))
    assert info["min_count"] == 8 < info["max_count"] <= 32 and np.isin(cnt, np.arange(8, 33, 4)).all()
    assert info["samples"] == int(cnt.sum()) and info["active_first"] == w * h
    assert info["passes"] == 1 + (info["max_count"] - 8) // 4
    assert info["rays_closest"] > info["samples"] and info["chunks"] >= info["passes"] and info["ms"] > 0.0
    # the same call through the binding: the tool's camera is (0, 3, 8) -> (0, 1, 0), fov 60
    r = sptr.Renderer(0)
    try:
        sptr.setup_default(r, "default_emitter")
        mine = r.render_adaptive(sptr.camera_lookat(aspect=w / h), w, h, 0.02, 8, 32, 4, max_depth=6)
        assert np.array_equal(r.read_sample_counts(), cnt.astype(np.uint32))
        assert np.array_equal(r.read_rgb8(), img)
        assert all(mine[k] == info[k] for k in ("samples", "rays_closest", "rays_shadow", "passes", "chunks"))
    finally:
        r.close()
    res = subprocess.run([exe, "--scene", "default_emitter", "--w", str(w), "--h", str(h), "--adaptive", "0.02", "--min-spp", "1",
                          "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "out of bounds" in res.stderr
