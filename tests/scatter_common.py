"""Scenes and ray sets shared by test_scatter_ref_cpu.py and test_gpu_scatter.py (test infrastructure, numpy only;
the float64 model is tests/scatter_ref.py).

A scene is analytic (rectangles and spheres with a material each, for the model) and is tessellated into a
FlatScene dict for the GPU and the oracle: every rectangle N x N quads of two triangles and a geometry of its own,
the spheres after them, so geomID -> material is exercised.  Vertices are float32-exact.

A ray set is a list of cameras on a scene: its rays are the cameras' primary rays of accumulation index 1 (the
oracle renders exactly those pixels; the GPU's ray path takes them as rays with the same rng states).  Pixels whose
path comes within DRAW_BORDER of a rectangle's edge or a sphere's silhouette are left out while the set is drawn,
so the model, with its margin of scatter_ref.BORDER, flags almost none of what is kept.  A frame set (frame_<scene>)
is every pixel of the 96 x 64 frame the render path is given, nothing left out.

  probes   16 panels and 2 spheres, 16 units apart, 13 materials; three cameras on each side of every panel
           (near-normal, oblique, and 2^-9 above the panel looking along it: incidence up to 89.9 degrees).
           Sets: metal, glass_panels, diffuse, spheres.
  glass    two rows of glass spheres (ior 1.5, 4 and 1.7) between a mirror floor and a mirror ceiling: refraction in, inside hits, out, to depth 6.
  slab     a diffuse floor and a diffuse emissive ceiling one unit apart, max albedo 0.75, open sides."""
import numpy as np

import env_common as E
import scatter_ref as R

f32, f64 = np.float32, np.float64
DRAW_BORDER = 0.01
MAX_DEPTH = 6
ENVS = E.SITE_CONFIGS  # (S, kind, (intensity, max_clamp)): noise at S = 3 and the coordinate map at S = 16


def material(albedo, metallic=0.0, ior=1.0, emission=(0.0, 0.0, 0.0), roughness=0.5):
    row = np.zeros(12, f32)
    row[0:3], row[3], row[4], row[5:8], row[8] = albedo, metallic, roughness, emission, ior
    return row


PROBE_MATERIALS = np.stack([
    material((0.9, 0.6, 0.3), metallic=0.51),                        # 0  metals
    material((0.3, 0.9, 0.6), metallic=0.75),                        # 1
    material((0.6, 0.3, 0.9), metallic=1.0),                         # 2
    material((1, 1, 1), ior=np.nextafter(f32(1.3), f32(2))),         # 3  glass: just transparent
    material((1, 1, 1), ior=1.5),                                    # 4
    material((1, 1, 1), ior=1.665),                                  # 5  tr just under its clamp
    material((1, 1, 1), ior=1.7),                                    # 6  tr at its clamp
    material((1, 1, 1), ior=4.0),                                    # 7
    material((0.8, 0.7, 0.6), ior=f32(1.3)),                         # 8  ior exactly 1.3: diffuse
    material((0.6, 0.7, 0.8), metallic=f32(0.1), ior=1.5),           # 9  metallic exactly 0.1f: diffuse
    material((1.0, 0.5, 0.25)),                                      # 10 diffuse, max albedo 1
    material((0.7, 0.6, 0.5)),                                       # 11 diffuse, max albedo below 1
    material((0.5, 0.5, 0.5), emission=(0.75, 0.75, 0.75)),          # 12 a grey emitter with an albedo
])
K_LO, K_HI = 3.0 / 64.0, 11.0 / 256.0  # normals (0, k, 1) / sqrt(1 + k^2): n.z = 0.998903 and 0.999078
ORIENT = {  # edge vectors (u, v), orthogonal and float32-exact; the normal is cross(u, v)
    "y": ((2, 0, 0), (0, 0, -2)),
    "z+": ((2, 0, 0), (0, 2, 0)),
    "z-": ((0, 2, 0), (2, 0, 0)),
    "x": ((0, 2, 0), (0, 0, 2)),
    "general": ((1, -1, 0.5), (1, 0.5, -1)),          # normal (1, 2, 2) / 3
    "tilt_lo": ((2, 0, 0), (0, 2, -2 * K_LO)),        # |n.z| just below 0.999: the z branch of the basis
    "tilt_hi": ((2, 0, 0), (0, 2, -2 * K_HI)),        # |n.z| just above: the y branch
}
PANELS = [("y", 0), ("general", 1), ("x", 2),
          ("z+", 3), ("general", 4), ("z-", 5), ("y", 6), ("x", 7),
          ("y", 8), ("z+", 9), ("z-", 10), ("x", 11), ("general", 10), ("tilt_lo", 11), ("tilt_hi", 10), ("tilt_lo", 12)]
PROBE_SPHERES = [(16, 2), (17, 11)]  # (grid slot, material)
PROBE_SETS = {"metal": range(0, 3), "glass_panels": range(3, 8), "diffuse": range(8, 16)}


def _slot(i):
    return np.array([16.0 * (i % 5), 0.0, -16.0 * (i // 5)])


def probe_scene():
    rects = []
    for i, (orient, mat) in enumerate(PANELS):
        u, v = (np.array(a, f64) for a in ORIENT[orient])
        rects.append((_slot(i) - 0.5 * u - 0.5 * v, u, v, mat))
    spheres = [(_slot(slot) + np.array([0.0, 1.0, 0.0]), 1.0, mat) for slot, mat in PROBE_SPHERES]
    return {"rects": rects, "spheres": spheres, "materials": PROBE_MATERIALS}


def glass_scene():
    mats = np.stack([material((0.75, 0.5, 0.25), metallic=1.0), material((1, 1, 1), ior=1.5), material((1, 1, 1), ior=4.0),
                     material((1, 1, 1), ior=1.7), material((0.5, 0.75, 0.25), metallic=0.75)])
    return {"rects": [(np.array([-4.0, 0.0, 4.0]), np.array([8.0, 0, 0]), np.array([0, 0, -8.0]), 0),
                      (np.array([-4.0, 2.75, 4.0]), np.array([8.0, 0, 0]), np.array([0, 0, -8.0]), 4)],
            "spheres": [(np.array([-1.25, 1.25, 0.0]), 1.0, 1), (np.array([1.25, 1.25, 0.0]), 1.0, 2),
                        (np.array([-1.25, 1.25, -2.5]), 1.0, 3), (np.array([1.25, 1.25, -2.5]), 1.0, 1)], "materials": mats}


def slab_scene():
    mats = np.stack([material((0.75, 0.5, 0.25)), material((0.5, 0.75, 0.25), emission=(1.0, 0.5, 0.25))])
    return {"rects": [(np.array([-4.0, 0.0, 4.0]), np.array([8.0, 0, 0]), np.array([0, 0, -8.0]), 0),
                      (np.array([-4.0, 1.0, 4.0]), np.array([8.0, 0, 0]), np.array([0, 0, -8.0]), 1)],
            "spheres": [], "materials": mats}


# name: (the analytic scene, N staged, N unstaged)
SCENES = {"probes": (probe_scene, 1, 8), "glass": (glass_scene, 4, 32), "slab": (slab_scene, 2, 32)}
_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = SCENES[name][0]()
    return _scenes[name]


def flat_scene(sc, N):
    """The FlatScene dict of an analytic scene: each rectangle N x N quads (N a power of two), one geometry each."""
    pos, idx, first, gm = [], [], [0], []
    nv = 0
    for p, u, v, mat in sc["rects"]:
        ga, gb = np.meshgrid(np.arange(N + 1) / N, np.arange(N + 1) / N, indexing="ij")
        q = np.asarray(p, f64)[None, :] + ga.ravel()[:, None] * np.asarray(u, f64) + gb.ravel()[:, None] * np.asarray(v, f64)
        i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        v00 = (i * (N + 1) + j).ravel()
        v10, v01, v11 = v00 + N + 1, v00 + 1, v00 + N + 2
        t = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)])
        idx.append(t + nv)
        pos.append(q)
        nv += len(q)
        first.append(first[-1] + len(t))
        gm.append(mat)
    p = np.concatenate(pos)
    assert (p.astype(f32) == p).all()
    sph = np.array([list(c) + [r] for c, r, _ in sc["spheres"]], f32).reshape(-1, 4)
    assert (sph == np.array([list(c) + [r] for c, r, _ in sc["spheres"]], f64).reshape(-1, 4)).all()
    gm += [mat for _, _, mat in sc["spheres"]]
    return {"positions": p.astype(f32), "indices": np.concatenate(idx).astype(np.uint32),
            "tri_geom_first": np.array(first, np.uint32), "spheres": sph, "geom_material": np.array(gm, np.uint32)}


# ---- cameras -----------------------------------------------------------------------------------------------------
def _panel_cameras(i):
    """(pos, target, fov) x 6: near-normal, oblique and grazing on either side of panel i."""
    u, v = (np.array(a, f64) for a in ORIENT[PANELS[i][0]])
    nh = np.cross(u, v)
    nh /= np.linalg.norm(nh)
    w = u if abs(u[1]) / np.linalg.norm(u) < abs(v[1]) / np.linalg.norm(v) else v  # the edge farther from the up axis
    half = 0.5 * np.linalg.norm(w)
    wh = w / np.linalg.norm(w)
    c = _slot(i)
    cams = []
    for s in (1.0, -1.0):
        cams.append((c + s * 3.0 * nh + 0.8 * wh, c, 50.0))
        cams.append((c + s * 0.6 * nh - 1.2 * half * wh, c + 0.5 * half * wh, 60.0))
        cams.append((c + s * 2.0 ** -9 * nh - 0.9 * half * wh, c + 0.3 * half * wh - s * 0.02 * nh, 4.0))
    return cams


def _sphere_cameras():
    return [(_slot(slot) + np.array([0.5, 1.5, 4.0]), _slot(slot) + np.array([0.0, 1.0, 0.0]), 30.0)
            for slot, _ in PROBE_SPHERES]


# the camera of the frame each scene is rendered with through the render path: (pos, target, fov)
RENDER_CAMERAS = {"probes": ((27.0, 5.0, -8.0), (24.0, 0.0, -24.0), 75.0),
                  "glass": ((0.0, 1.5, 3.75), (0.0, 1.25, -1.0), 45.0),
                  "slab": ((2.0, 0.5, 0.0), (4.0, 0.45, 0.5), 90.0)}


# set: (scene, [(pos, target, fov)], W, H)
def set_specs():
    specs = {name: ("probes", [cam for i in panels for cam in _panel_cameras(i)], 16, 12)
             for name, panels in PROBE_SETS.items()}
    specs["spheres"] = ("probes", _sphere_cameras(), 40, 30)
    specs["glass"] = ("glass", [RENDER_CAMERAS["glass"]], 64, 48)
    specs["slab"] = ("slab", [RENDER_CAMERAS["slab"]], 64, 48)
    return specs


SET_NAMES = ("metal", "glass_panels", "diffuse", "spheres", "glass", "slab")
FRAME_W, FRAME_H = 96, 64
FRAME_NAMES = ("frame_probes", "frame_glass", "frame_slab")
class RaySet:
    """The kept pixels of a set's cameras: per camera the oracle camera array and the pixel indices, and over all
    of them origins (n, 3), float32 dirs (n, 3) and rng states (n,)."""

    def __init__(self, name, scene_name, cams, W, H, keep_all=False):
        import oracle

        self.name, self.scene_name, self.W, self.H = name, scene_name, W, H
        self.cams, self.pixels = [], []
        o, d, s = [], [], []
        sc = scene(scene_name)
        env = (E.env_map("coordinate", 2), 1.0, 1e30)
        for pos, target, fov in cams:
            cam = oracle.camera(pos=tuple(f32(pos)), target=tuple(f32(target)), fov=fov, aspect=W / H)
            dirs, rng = oracle.primary(cam, W, H, 1)
            dirs, rng = dirs.reshape(-1, 3), rng.ravel()
            drop = R.trace(sc, cam[:3], dirs, rng, env, MAX_DEPTH, border=DRAW_BORDER)["fragile"]
            keep = np.arange(len(dirs)) if keep_all else np.flatnonzero(~drop)
            self.cams.append(cam)
            self.pixels.append(keep.astype(np.uint32))
            o.append(np.broadcast_to(cam[:3].astype(f64), (len(keep), 3)))
            d.append(dirs[keep])
            s.append(rng[keep])
        self.origins, self.dirs, self.states = np.concatenate(o), np.concatenate(d), np.concatenate(s)
        for a in (self.origins, self.dirs, self.states):
            a.setflags(write=False)
        self._model, self._oracle = {}, {}

    def __len__(self):
        return len(self.dirs)

    def rays(self):
        r = np.zeros((len(self), 8), f32)
        r[:, 0:3], r[:, 3:6] = self.origins, self.dirs
        return r

    def model(self, env_index, depth=MAX_DEPTH, mutant=None, du_underived=None):
        key = (env_index, depth, mutant, du_underived)
        if key not in self._model:
            S, kind, state = ENVS[env_index]
            self._model[key] = R.trace(scene(self.scene_name), self.origins, self.dirs, self.states,
                                       (E.env_map(kind, S), state[0], state[1]), depth, mutant=mutant,
                                       du_underived=du_underived)
        return self._model[key]

    def oracle(self, env_index, depth=MAX_DEPTH):
        """(radiance (n, 3) float32, closest-hit queries) of the float32 oracle on the set's pixels, no lights."""
        import oracle

        key = (env_index, depth)
        if key not in self._oracle:
            S, kind, state = ENVS[env_index]
            P = prepared(self.scene_name)
            mats = scene(self.scene_name)["materials"]
            out, closest = [], 0
            for cam, pix in zip(self.cams, self.pixels):
                acc, _, cnt = P.render(cam, self.W, self.H, mats, np.zeros((0, 8), f32), frames=1, max_depth=depth,
                                       threads=1, env_faces=E.env_map(kind, S), env_intensity=state[0], env_clamp=state[1],
                                       pixels=pix)
                assert cnt["rays_shadow"] == 0
                out.append(acc.reshape(-1, 3)[pix])
                closest += cnt["rays_closest"]
            self._oracle[key] = (np.concatenate(out), closest)
        return self._oracle[key]

    def granted_du(self, env_index, depth=MAX_DEPTH):
        """What the underived rays of the set are granted: 4 x the oracle's worst needed du, not below 16 eps."""
        need = R.needed_du(self.oracle(env_index, depth)[0], self.model(env_index, depth))
        return R.granted_du(need), need

    def bound(self, env_index, depth=MAX_DEPTH):
        """The model's result with the set's tolerance complete: derived, and granted where it is not."""
        if not self.model(env_index, depth)["underived"].any():
            return self.model(env_index, depth)
        return self.model(env_index, depth, du_underived=self.granted_du(env_index, depth)[0])


_sets, _prepared = {}, {}


def prepared(scene_name):
    import oracle

    if scene_name not in _prepared:
        _prepared[scene_name] = oracle.Prepared(flat_scene(scene(scene_name), SCENES[scene_name][1]))
    return _prepared[scene_name]


def ray_set(name):
    if name not in _sets:
        if name.startswith("frame_"):  # every pixel of the frame the render path is given
            sc = name[len("frame_"):]
            _sets[name] = RaySet(name, sc, [RENDER_CAMERAS[sc]], FRAME_W, FRAME_H, keep_all=True)
        else:
            _sets[name] = RaySet(name, *set_specs()[name])
    return _sets[name]
