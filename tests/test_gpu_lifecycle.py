"""GPU: contexts created, used and destroyed over and over.  Every device buffer, event, stream and graph of
a context is held by an owner that frees it (csrc/dev_owned.h), and ~sptr_ctx waits for the context's work
first; here each round reaches every owner — dynamic upload (refit state), a timed denoised render (wave
buffers, cull, the event pool, AOV planes, the filter's images), a refit, sorted and unsorted ray queries
from host pointers (sort scratch, staging), the legacy query (qbuf), and the lane context every sptr_create
makes — and must give the same bytes as the first.  The leak accounting itself is tests/cpp/test_dev_owned.cpp's:
free device memory moves for reasons outside this process, so nothing here asserts on it.

Every binding method raises SptrError unless its call returned SPTR_OK."""
import numpy as np
import pytest

import sptr

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, NRAYS = 64, 48, 2, 4, 256


def _rays():
    g = np.random.default_rng(7)
    o = np.tile(np.float32([0.0, 3.0, 8.0]), (NRAYS, 1))
    target = np.stack([g.uniform(-4, 4, NRAYS), g.uniform(-1, 4, NRAYS), g.uniform(-3, 3, NRAYS)], axis=1)  # some miss
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.zeros((NRAYS, 1)), np.full((NRAYS, 1), 1e30)], axis=1).astype(np.float32)


def _use(r):
    """One context's whole use; returns its outputs as bytes, by name."""
    r.set_dynamic(True)
    s = sptr.setup_default(r, "default")
    r.set_denoise(iterations=2)
    cam = sptr.camera_lookat(aspect=W / H)
    r.render(cam, W, H, spp=SPP, max_depth=DEPTH, flags=sptr.SPTR_FRAME_TIMING)
    out = {"rgb8": r.read_rgb8(), "denoised": r.read_denoised(), "aov_id": r.read_aov(sptr.SPTR_AOV_ID)}
    r.update_geometry(positions=s.positions)  # the unchanged positions: the same scene, refitted
    assert r.refit_info()["refits"] == 1
    rays = _rays()
    q = r.query_rays(rays, sort=True)
    out.update({"q_" + k: v for k, v in q.items()})
    out["occluded"] = r.query_rays(rays, any_hit=True, sort=False)["occluded"]
    geom, prim, t, ng = r.intersect(rays)
    out.update({"i_geom": geom, "i_prim": prim, "i_t": t, "i_ng": ng})
    hit = q["geom"] != 0xFFFFFFFF
    assert 0 < hit.sum() < NRAYS  # hits and misses both
    assert np.array_equal(geom, q["geom"]) and np.array_equal(out["occluded"] != 0, hit)
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


def _render_bytes(r):
    r.render(sptr.camera_lookat(aspect=W / H), W, H, spp=SPP, max_depth=DEPTH)
    return r.read_rgb8().tobytes(), r.read_denoised().tobytes()


def test_create_use_destroy_rounds():
    first = None
    for _ in range(3):
        r = sptr.Renderer(0)
        try:
            got = _use(r)
        finally:
            r.close()
        if first is None:
            first = got
        assert got.keys() == first.keys()
        for k in first:
            assert got[k] == first[k], k


def test_a_context_outlives_its_neighbour():
    a, b = sptr.Renderer(0), sptr.Renderer(0)
    try:
        ua, ub = _use(a), _use(b)
        assert ua == ub
        before = _render_bytes(b)
        assert _render_bytes(a) == before
        a.close()
        assert _render_bytes(b) == before
    finally:
        a.close()
        b.close()
