"""Yardstick of environment.composite_environment: the module's formula in plain torch with explicit index gathers,
meant for CPU tensors in float64 (it runs on any device and dtype: the float32 composition on the device is the same
function; its backward is autograd's), an explicit per-pixel Python loop the yardstick is checked against, the cameras
of the tests, seeded cases, and the pixels close to a face edge that comparisons leave out."""
import math

import torch

from taichi_gaussian_rasterizer_amd import CameraParams

TRANSLATION = (0.3, -1.2, 2.0)
OTHERS = ((1, 2), (0, 2), (0, 1))  # the two other axes of a face's axis, ascending


def view_directions(camera, dtype=None):
    """(H, W, 3): d = Rcw^T ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) for every pixel"""
    W, H = camera.image_size
    proj, T = camera.projection, camera.T_camera_world
    if dtype is not None:
        proj, T = proj.to(dtype), T.to(dtype)
    x = torch.arange(W, dtype=proj.dtype, device=proj.device)
    y = torch.arange(H, dtype=proj.dtype, device=proj.device)
    dx = ((x + 0.5 - proj[2]) / proj[0]).view(1, W).expand(H, W)
    dy = ((y + 0.5 - proj[3]) / proj[1]).view(H, 1).expand(H, W)
    d_cam = torch.stack([dx, dy, torch.ones_like(dx)], dim=-1)
    return d_cam @ T[:3, :3]  # row vectors: d_i = sum_j Rcw[j, i] d_cam_j


def lookup(directions, R):
    """face (long), v, u (clamped texel coordinates) of (..., 3) directions"""
    mag = directions.abs()
    axis = mag.argmax(dim=-1)  # the first of equal maxima
    d_a = directions.gather(-1, axis[..., None])[..., 0]
    face = 2 * axis + (d_a < 0).long()
    first = torch.tensor([o[0] for o in OTHERS], device=directions.device)[axis]
    second = torch.tensor([o[1] for o in OTHERS], device=directions.device)[axis]
    p = directions.gather(-1, first[..., None])[..., 0] / d_a.abs()
    q = directions.gather(-1, second[..., None])[..., 0] / d_a.abs()
    u = ((p + 1) / 2 * R - 0.5).clamp(0, R - 1)
    v = ((q + 1) / 2 * R - 0.5).clamp(0, R - 1)
    return face, v, u


def sky_reference(env, camera):
    R = env.shape[1]
    face, v, u = lookup(view_directions(camera, env.dtype), R)
    i0, j0 = u.floor().long().clamp(max=R - 1), v.floor().long().clamp(max=R - 1)
    i1, j1 = (i0 + 1).clamp(max=R - 1), (j0 + 1).clamp(max=R - 1)
    fu, fv = (u - i0)[..., None], (v - j0)[..., None]
    top = env[face, j0, i0] + (env[face, j0, i1] - env[face, j0, i0]) * fu
    bot = env[face, j1, i0] + (env[face, j1, i1] - env[face, j1, i0]) * fu
    return top + (bot - top) * fv


def composite_reference(env, image, image_weight, camera):
    sky = sky_reference(env, camera)
    if image is None:
        return sky
    return image + (1 - image_weight)[..., None] * sky


def composite_loop(env, image, image_weight, camera):
    """the formula of the module docstring, pixel by pixel, in Python floats (float64)"""
    R, C = env.shape[1], env.shape[3]
    W, H = camera.image_size
    fx, fy, cx, cy = (float(v) for v in camera.projection.double())
    Rcw = camera.T_camera_world.double()[:3, :3].tolist()
    out = torch.zeros(H, W, C, dtype=torch.float64)
    for y in range(H):
        for x in range(W):
            d_cam = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1.0)
            d = [sum(Rcw[j][i] * d_cam[j] for j in range(3)) for i in range(3)]
            a = 0
            for k in (1, 2):
                if abs(d[k]) > abs(d[a]):
                    a = k
            face = 2 * a + (1 if d[a] < 0 else 0)
            p, q = (d[k] / abs(d[a]) for k in OTHERS[a])
            u = min(max((p + 1) / 2 * R - 0.5, 0.0), R - 1.0)
            v = min(max((q + 1) / 2 * R - 0.5, 0.0), R - 1.0)
            i0, j0 = min(int(math.floor(u)), R - 1), min(int(math.floor(v)), R - 1)
            i1, j1 = min(i0 + 1, R - 1), min(j0 + 1, R - 1)
            fu, fv = u - i0, v - j0
            e = env[face].double()
            top = e[j0, i0] + (e[j0, i1] - e[j0, i0]) * fu
            bot = e[j1, i0] + (e[j1, i1] - e[j1, i0]) * fu
            sky = top + (bot - top) * fv
            out[y, x] = sky if image is None else image[y, x].double() + (1 - float(image_weight[y, x])) * sky
    return out


def grads_of(fn, env, image, image_weight, camera, upstream):
    """value, d_env, d_image_weight of sum(fn(...) * upstream); image_weight may be None with image"""
    e = env.detach().clone().requires_grad_(True)
    w = None if image_weight is None else image_weight.detach().clone().requires_grad_(True)
    out = fn(e, image, w, camera)
    (out * upstream).sum().backward()
    return out.detach(), e.grad, None if w is None else w.grad


# ------------------------------------------------------------------------------------------------------- cameras
def rotation(axis, angle):
    """Rodrigues, float64"""
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def make_camera(size, intrinsics, rot, translation=TRANSLATION, dtype=torch.float64):
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = rot
    T[:3, 3] = torch.as_tensor(translation, dtype=torch.float64)
    return CameraParams(projection=torch.as_tensor(intrinsics, dtype=torch.float64).to(dtype), T_camera_world=T.to(dtype),
                        near_plane=0.1, far_plane=100.0, image_size=tuple(size))


def _specs():
    eye = torch.eye(3, dtype=torch.float64)
    return {
        "seam": ((53, 37), (40, 42, 26.1, 18.3), rotation((1, 2, 3), 0.9)),
        "corner": ((64, 130), (30, 30, 32, 65),
                   rotation((-1, 1, 0), math.acos(1 / math.sqrt(3))) @ rotation((0, 0, 1), 0.3)),
        "wide": ((96, 64), (12, 12, 48, 32), rotation((3, -1, 2), 2.1)),
        "tele": ((64, 64), (2000, 2000, 32, 32), rotation((0, 1, 0), math.pi / 4 + 1e-3)),
        "one": ((1, 1), (1.0, 1.0, 0.5, 0.5), eye),
        "small": ((5, 6), (4.0, 5.0, 2.4, 3.1), eye),
    }


CAMERAS = tuple(_specs())


def camera(name, dtype=torch.float64, translation=TRANSLATION):
    size, intrinsics, rot = _specs()[name]
    return make_camera(size, intrinsics, rot, translation, dtype)


def faces_seen(cam, R=8):
    return sorted(set(lookup(view_directions(cam, torch.float64), R)[0].flatten().tolist()))


def kept_pixels(cam, margin=1e-4):
    """bool (H, W): the pixels whose two largest |d_i| (float64) differ by at least `margin` relative to the largest --
    the output is discontinuous across a face edge, where rounding may choose the other face"""
    mag = view_directions(cam, torch.float64).abs().sort(dim=-1, descending=True).values
    return (mag[..., 0] - mag[..., 1]) >= margin * mag[..., 0]


def random_case(name, R, C, seed=0, dtype=torch.float64):
    """camera, env, image, image_weight, upstream and the kept pixels: uniform noise, weights in [0, 1]; the upstream
    gradient is zero and the weight one at the pixels left out, so that d_env compares in full"""
    cam = camera(name, dtype)
    W, H = cam.image_size
    gen = torch.Generator().manual_seed(seed)
    env = torch.rand(6, R, R, C, generator=gen, dtype=torch.float64)
    image = torch.rand(H, W, C, generator=gen, dtype=torch.float64)
    weight = torch.rand(H, W, generator=gen, dtype=torch.float64)
    upstream = torch.rand(H, W, C, generator=gen, dtype=torch.float64) - 0.5
    keep = kept_pixels(cam)
    weight[~keep] = 1.0
    upstream[~keep] = 0.0
    return cam, env.to(dtype), image.to(dtype), weight.to(dtype), upstream.to(dtype), keep
