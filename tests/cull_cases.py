"""Inputs for the tests of the conservative culls (tests/test_cull_bound.py, tests/test_gpu_cull_bounds.py): geometry and cameras a
footprint bound has to survive.  Inputs only -- no expected values, no device, no torch.

The culls (cull_key's band test, box_live's, the two-pass gate per box and per splat) bound a splat's reach on screen by
|J_row|^2 (1 + tr^2) * view_scale2 * rho^2 lambda_max(Sigma); a bound that is too small loses one splat of one frame, silently.
hostile_attrs is a cloud of the splats such a bound is worst at, wall_attrs an occluder that lets pass 1 of a two-pass frame
finish bins, CAMERAS the views: rigid, similarities, cameras that are no rotation at all, wide / long / asymmetric frusta, an
offset viewport and an eye inside the cloud."""
import math

import numpy as np

from splatapult_amd import camera, synthetic

N, W, H = 4097, 352, 300          # 17 cull boxes, the last with one splat; 11 x 10 bins, the top row 12 px high
SEEDS = (41, 42)
Z0 = 7.0                          # the default camera sits at (0, 0, Z0) and looks down -z
NF = [camera.Z_NEAR, camera.Z_FAR]


def hostile_attrs(n=N, seed=SEEDS[0], aspect=W / H):
    """synthetic.generate's attributes with, slice by slice (n // 32 splats each): needles (one log-scale +4, one -2) turned at
    random; needles along world x, y, z in turn (identity rotation); sheets (two long axes); giants (log-scale +3); zero
    covariance (log-scale -40) at opacity 30; opacity straddling alpha = 1/256; alpha == 1; centres with |ndc.y| and with |ndc.x|
    in [1.3, 1.5) for the default camera at z = Z0 (aspect: the viewport's W / H); centres around the ndc.z = 0.25 plane; exact
    duplicates.  Last, a giant at every upload index = 0 mod 256: one member sets the footprint bound of its whole cull box."""
    a = synthetic.generate(n, seed=seed, pos_sigma=2.5, log_scale_mean=-3.0, log_scale_sigma=1.0, workers=1)
    xyz, ls, op, rot = a["xyz"], a["log_scale"], a["opacity"], a["rot"]
    k = max(n // 32, 1)
    s = lambda j: slice(j * k, (j + 1) * k)
    ident = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    ls[s(0), 0] += 4.0                                       # needles, random rotations
    ls[s(0), 1] -= 2.0
    axis = np.arange(k) % 3                                  # needles along world x, y, z
    rot[s(1)] = ident
    ls[s(1)] = ls[s(1)] + np.where(np.arange(3)[None, :] == axis[:, None], 4.0, -2.0).astype(np.float32)
    ls[s(2), 0] += 2.5                                       # sheets
    ls[s(2), 1] += 2.5
    ls[s(2), 2] -= 2.0
    ls[s(3)] += 3.0                                          # giants
    ls[s(4)] = -40.0                                         # zero covariance: the 0.3 px low-pass term alone
    op[s(4)] = 30.0
    op[s(5)] = np.linspace(-5.7, -5.3, k)                    # alpha = 1/256 is the logit -5.54
    op[s(6)] = 30.0                                          # alpha == 1
    t = math.tan(0.5 * camera.FOVY)
    u = np.linspace(1.3, 1.5, k, endpoint=False) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    xyz[s(7), 1] = u * (Z0 - xyz[s(7), 2]) * t               # in the guard band, where tr is largest
    xyz[s(8), 0] = u * (Z0 - xyz[s(8), 2]) * t * aspect
    xyz[s(9), 2] = Z0 - np.linspace(0.05, 0.5, k)            # around the ndc.z = 0.25 plane (depth 0.2667)
    for key in a:                                            # exact duplicates: equal depth keys, equal everything
        if a[key] is not None:
            a[key][s(10)] = a[key][s(11)]
    ls[::256] = 0.0                                          # one giant (the mean log-scale + 3) per 256 upload indices
    op[::256] = 2.0
    return a


def wall_attrs(k=512, layers=4):
    """k large, near-opaque splats in `layers` sheets at z = 4.0 ... in front of the left half of the default view (camera at
    z = Z0): pass 1 of a two-pass frame finishes the bins over them"""
    per = [k // layers + (1 if i < k % layers else 0) for i in range(layers)]
    xyz = np.empty((k, 3), np.float32)
    at = 0
    for i, m in enumerate(per):
        cols = max(int(math.ceil(math.sqrt(m * 1.6 / 3.0))), 1)
        rows = (m + cols - 1) // cols
        j = np.arange(m)
        xyz[at:at + m, 0] = -1.7 + 1.6 * ((j % cols) + 0.5 * (i % 2)) / cols
        xyz[at:at + m, 1] = -1.5 + 3.0 * ((j // cols) + 0.5) / rows
        xyz[at:at + m, 2] = 4.0 + 0.15 * i
        at += m
    f_dc = np.linspace(-1.0, 1.0, k * 3, dtype=np.float32).reshape(k, 3)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (k, 1))
    return dict(xyz=xyz, f_dc=f_dc, f_rest=np.zeros((k, 45), np.float32), opacity=np.full(k, 6.0, np.float32),
                log_scale=np.full((k, 3), math.log(0.22), np.float32), rot=rot)


def join_attrs(a, b):
    return {key: np.concatenate([a[key], b[key]], axis=0) for key in a}


# ---- cameras -----------------------------------------------------------------------------------------------------------------

def _roll(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _mat3_times(cam, A):
    """the camera-to-world matrix with its upper-left 3x3 (rows x columns) multiplied by A from the right: camera axes A"""
    m = np.asarray(cam, np.float64).reshape(4, 4).T.copy()
    m[:3, :3] = m[:3, :3] @ np.asarray(A, np.float64)
    return m.T.astype(np.float32).reshape(16).copy()


def _orbit(yaw, pitch, radius=Z0):
    """camera.pose turned by yaw and pitch about the origin: the cloud stays in the middle of the view"""
    cam = camera.pose((0.0, 0.0, 0.0), yaw, pitch).reshape(4, 4).copy()          # cam[c] = column c
    cam[3, :3] = radius * cam[2, :3]
    return cam.reshape(16)


def _view(cam, W, H, proj=None, viewport=None):
    return cam, proj if proj is not None else camera.perspective(camera.FOVY, W / H), viewport or [0, 0, W, H], NF


def _shear():
    A = np.eye(3)
    A[1, 0] = 0.5                                            # I + 0.5 e1 e0^T
    return A


CAMERAS = {
    "rigid_pitched": lambda W, H: _view(_orbit(0.4, -0.35), W, H),
    "rolled": lambda W, H: _view(_mat3_times(camera.pose((0.0, 0.0, Z0)), _roll(math.radians(30.0))), W, H),
    "similarity_small": lambda W, H: _view(_mat3_times(camera.pose((0.0, 0.0, Z0)), 0.37 * np.eye(3)), W, H),
    "similarity_big": lambda W, H: _view(_mat3_times(camera.pose((0.0, 0.0, Z0)), 3.0 * np.eye(3)), W, H),
    "squashed": lambda W, H: _view(_mat3_times(_orbit(math.radians(45.0), 0.0), _roll(math.radians(45.0)) @ np.diag([1.0, 0.5, 1.0])), W, H),
    "stretched_depth": lambda W, H: _view(_mat3_times(_orbit(0.3, -0.2), np.diag([1.0, 1.0, 2.5])), W, H),
    "sheared": lambda W, H: _view(_mat3_times(_orbit(0.3, -0.2), _shear()), W, H),
    "wide": lambda W, H: _view(camera.pose((0.0, 0.0, Z0)), W, H, proj=camera.perspective(math.radians(100.0), W / H)),
    "long": lambda W, H: _view(camera.pose((0.0, 0.0, 12.0)), W, H, proj=camera.perspective(math.radians(20.0), W / H)),
    "asymmetric": lambda W, H: _view(camera.pose((0.0, 0.0, Z0 - 2.0), 0.2), W, H, proj=camera.create_projection(-1.0, 0.8, 0.95, -0.95)),
    "offset_viewport": lambda W, H: _view(camera.pose((0.0, 0.0, Z0), 0.1), W, H, viewport=[13, 37, W, H]),
    "inside": lambda W, H: _view(camera.pose((0.3, 0.2, 0.5), 1.3, 0.2), W, H),
}
CAMERA_NAMES = ("rigid_pitched", "rolled", "similarity_small", "similarity_big", "squashed", "stretched_depth", "sheared", "wide",
                "long", "asymmetric", "offset_viewport", "inside")
assert tuple(CAMERAS) == CAMERA_NAMES

LAYOUTS = (("contiguous", 1, 8), ("interleaved", 1, 3), ("block", 2, 4))      # (kind, block rows, ranks)
