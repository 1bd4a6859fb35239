"""Shared scene builders for the parity tests (inputs only; no expected values live here)."""
import numpy as np

from splatapult_amd import camera, synthetic
from splatapult_amd.scene import GaussianCloud

NF = [camera.Z_NEAR, camera.Z_FAR]


def synth_cloud(n, seed, full_sh=True, **kw):
    return synthetic.make_cloud(n, seed=seed, full_sh=full_sh, **kw)


def hard_attrs(n=3000, seed=11):
    """Synthetic attributes with the nasty cases mixed in: splats behind the camera, outside the
    1.5 cull band and the 2.0 guard band, nearer than the ndc.z<0.25 plane, beyond the far plane,
    huge and needle-thin splats, alpha ~ 0 and alpha ~ 1, exact duplicates (equal depth keys)."""
    a = synthetic.generate(n, seed=seed, pos_sigma=2.5, log_scale_mean=-3.0, log_scale_sigma=1.0)
    xyz, ls, op = a["xyz"], a["log_scale"], a["opacity"]
    k = n // 20
    xyz[0:k, 2] += 9.0                       # behind / very near a camera sitting at z = 7
    xyz[k:2 * k, 0] *= 6.0                   # far off to the side
    xyz[2 * k:3 * k, 2] = 7.0 - np.linspace(0.05, 0.5, k)      # around the ndc.z = 0.25 plane (depth 0.2667)
    xyz[3 * k:4 * k, 2] = 7.0 - np.linspace(900.0, 1100.0, k)  # around the far plane
    ls[4 * k:5 * k] += 3.0                   # huge
    ls[5 * k:6 * k, 0] += 2.5                # needles
    ls[5 * k:6 * k, 1] -= 2.0
    op[6 * k:7 * k] = -9.0                   # alpha < 1/256
    op[7 * k:8 * k] = 30.0                   # alpha == 1
    op[8 * k:9 * k] = np.linspace(-5.7, -5.3, k)   # straddles alpha = 1/256 (logit -5.54)
    xyz[9 * k:10 * k] = xyz[10 * k:11 * k]   # duplicates -> identical keys, tie order matters
    return a


def cloud_from_attrs(a, full_sh=True):
    gc = GaussianCloud(GaussianCloud.Options(full_sh, full_sh))
    assert gc.FromAttributes(a["xyz"], a["f_dc"], a["f_rest"] if full_sh else None, a["opacity"], a["log_scale"],
                             a["rot"])
    return gc


def default_view(W, H, z=7.0, yaw=0.0, pitch=0.0, x=0.0, y=0.0):
    cam = camera.pose((x, y, z), yaw, pitch)
    proj = camera.perspective(camera.FOVY, W / H)
    return cam, proj, [0, 0, W, H], NF


def strip_view(W, H, yaw=0.0):
    """a W x H crop around the centre of an 8192 x 8192, 90-degree frame (focal length 4096 px on both axes) seen from z = 7:
    8192 x 64 and 64 x 8192 have 256 bins along one axis and 2 along the other"""
    cam = camera.pose((0.0, 0.0, 7.0), yaw, 0.0)
    proj = camera.create_projection(-W / 8192.0, W / 8192.0, H / 8192.0, -H / 8192.0)
    return cam, proj, [0, 0, W, H], NF


def strip_attrs(n, seed, W, H, hard):
    """attributes of a cloud that lies inside the strip of strip_view(W, H): hard_attrs or a plain synthetic cloud whose
    coordinate along the strip's short axis is scaled by min / max of the viewport's sides"""
    a = hard_attrs(n, seed) if hard else synthetic.generate(n, seed=seed, pos_sigma=2.5, log_scale_mean=-3.6)
    a["xyz"][:, 1 if W > H else 0] *= min(W, H) / max(W, H)
    return a
