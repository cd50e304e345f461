"""A learnable cubemap environment (sky) behind the render (HIP).

    composite_environment(env, image, image_weight, camera) -> (H, W, C): the render over the sky
    sample_environment(env, camera)                         -> (H, W, C): the sky alone
    environment_directions(R, device, dtype)                -> (6, R, R, 3): the direction of every texel centre
    constant_environment(colour, R)                         -> (6, R, R, C): one colour everywhere

Outdoor captures need a model of what lies behind the Gaussians.  `env` is that model: a (6, R, R, C) map, channel-last
and contiguous, C in 1 .. 4, usually an nn.Parameter, looked up by the view direction of every pixel.  A trainer renders
with `render_gaussians(..., differentiable_weight=True)` and composites `Rendering.image` and `Rendering.image_weight`
over the map before the loss; the weight's gradient then tells the Gaussians how much sky they hide.

`image` is (H, W, C) and `image_weight` (H, W), both read through their strides (`Rendering.image`, or a channel slice
of a wider render, goes in without a copy); (W, H) = camera.image_size.  The kernels read `camera.projection` and
`camera.T_camera_world` on the device: nothing is read back and the host never waits.  For the pixel at column x, row
y (pixel centres at + 0.5, as in the rasterizer):

    d_cam = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)
    d     = Rcw^T d_cam           Rcw = T_camera_world[:3, :3], taken as a rotation; the map is at infinity, the
                                  translation is not read
    a     = the axis of the largest |d_i|, ties to the lower index;   face = 2 a + (d_a < 0)
    (p, q) = the two other components in ascending axis order, divided by |d_a|    (a=0: y,z   a=1: x,z   a=2: x,y)
    u = clamp((p + 1) / 2 * R - 0.5, 0, R - 1)   column        v = clamp((q + 1) / 2 * R - 0.5, 0, R - 1)   row
    sky = bilinear interpolation of env[face] at (v, u)    (taps clamped inside the face; R = 1: one texel per face)
    out = image + (1 - image_weight) * sky

which is grid_sample(bilinear, border, align_corners=False) on the chosen face.  The convention is this module's own:
faces 0 .. 5 are +x, -x, +y, -y, +z, -z in WORLD axes, a face's column runs along the lower and its row along the
higher of its two other axes, with no sign flips from face to face -- `environment_directions` is the way to fill a
map from an equirectangular photo or any function of direction.  There is no filtering across face seams: at a face
edge the taps clamp to the face, so a map is continuous across a seam only as far as its two faces agree there.

Gradients: d_image is the incoming gradient itself; d_image_weight = -sum_c grad_c sky_c; d_env is dense, exactly zero
where no pixel looks, and -- like every output here -- repeats bit for bit from run to run: it is a gather with one
fixed-order sum per texel, no atomics (csrc/envmap.hip).  The view direction is NOT differentiated: `projection` and
`T_camera_world` get no gradient from the sky; poses take theirs through the Gaussians.  Each gradient is computed only
when asked for.  Limits: pinhole cameras, C <= 4, R <= 16384, no gradient to the pose, no seam filtering.  float32, or
float64 when every tensor of the call -- the camera's two included -- is float64 (gradcheck).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native as nv
from .losses import _strided, _strided_mask
from .perspective import CameraParams

__all__ = ["composite_environment", "sample_environment", "environment_directions", "constant_environment"]

MAX_CHANNELS = 4
MAX_EDGE = 16384


def _check(what, env, image, image_weight, camera):
    """every argument error, cheapest first and all before any launch; returns the dtype"""
    if not isinstance(env, torch.Tensor):
        raise TypeError(f"{what}: env must be a torch.Tensor, got {type(env).__name__}")
    if not isinstance(camera, CameraParams):
        raise TypeError(f"{what}: camera must be a CameraParams, got {type(camera).__name__}")
    if env.dim() != 4 or env.shape[0] != 6 or env.shape[1] != env.shape[2] or env.shape[1] < 1:
        raise ValueError(f"{what}: env must be (6, R, R, C) with R >= 1, got {tuple(env.shape)}")
    R, C = int(env.shape[1]), int(env.shape[3])
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{what}: env has {C} channels; 1 to {MAX_CHANNELS} are supported")
    if R > MAX_EDGE:
        raise ValueError(f"{what}: env edge {R} above {MAX_EDGE}")
    W, H = (int(v) for v in camera.image_size)
    if W < 1 or H < 1:
        raise ValueError(f"{what}: camera.image_size {camera.image_size} is empty")
    if (image is None) != (image_weight is None):
        raise ValueError(f"{what}: image and image_weight go together (both, or both None for the sky alone)")
    if image is not None:
        for name, t in (("image", image), ("image_weight", image_weight)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if image.dim() != 3 or image.shape[2] != C:
            raise ValueError(f"{what}: image must be (H, W, {C}) for an env {tuple(env.shape)}, got {tuple(image.shape)}")
        if tuple(image.shape[:2]) != (H, W):
            raise ValueError(f"{what}: image {tuple(image.shape)} does not match camera.image_size (W, H) = {(W, H)}")
        if tuple(image_weight.shape) != (H, W):
            raise ValueError(f"{what}: image_weight {tuple(image_weight.shape)} for an image {tuple(image.shape)}: "
                             f"expected {(H, W)}")
    tensors = (env, image, image_weight, camera.projection, camera.T_camera_world)
    dtypes = {t.dtype for t in tensors if t is not None}
    if len(dtypes) != 1 or not dtypes <= {torch.float32, torch.float64}:
        raise TypeError(f"{what}: every tensor, the camera's two included, must be float32, or every one float64; got "
                        f"{', '.join(str(t.dtype) for t in tensors if t is not None)}")
    return nv.float_dtype(*tensors, what=what)


class _Call:
    """one map, frame and camera prepared for the C-ABI: views, strides, the entry points of the dtype"""

    def __init__(self, env, image, image_weight, camera, dtype):
        self.env = env.detach().contiguous()
        self.R, self.C = int(env.shape[1]), int(env.shape[3])
        self.W, self.H = (int(v) for v in camera.image_size)
        self.projection = camera.projection.detach().contiguous()
        self.pose = camera.T_camera_world.detach().contiguous()
        self.image, image_args = None, (None, 0, 0)
        self.weight, self.weight_args = None, (None, 0, 0)
        if image is not None:
            self.image, _, isr, isp = _strided(image.detach())
            self.weight, _, wsr, wsp = _strided_mask(image_weight.detach(), dtype)
            image_args = (nv.ptr(self.image), isr, isp)
            self.weight_args = (nv.ptr(self.weight), wsr, wsp)
        self.dtype = dtype
        self.f64 = dtype == torch.float64
        suffix = "_f64" if self.f64 else ""
        self.fwd_name, self.bwd_name = "gs_envmap_fwd" + suffix, "gs_envmap_bwd" + suffix
        self.head = (self.H, self.W, self.C, nv.ptr(self.env), self.R)
        self.fwd_args = (*self.head, *image_args, *self.weight_args, nv.ptr(self.projection), nv.ptr(self.pose))

    def forward(self):
        out = torch.empty((self.H, self.W, self.C), dtype=self.dtype, device=self.env.device)
        nv.check(getattr(nv.lib(), self.fwd_name)(*self.fwd_args, nv.ptr(out), nv.stream()), self.fwd_name)
        return out

    def backward(self, grad_out, want_env, want_weight):
        dev = self.env.device
        if nv.float_dtype(grad_out, what=self.bwd_name) != self.dtype:
            raise TypeError(f"{self.bwd_name}: {self.dtype} forward, {grad_out.dtype} gradient")
        grad_out = grad_out.reshape(self.H, self.W, self.C).contiguous()
        d_weight = torch.empty((self.H, self.W), dtype=self.dtype, device=dev) if want_weight else None
        d_env, scratch, nbytes = None, None, 0
        if want_env:
            d_env = torch.empty(self.env.shape, dtype=self.dtype, device=dev)
            nbytes = nv.lib().gs_envmap_scratch_bytes(self.H, self.W, self.C, self.R, int(self.f64))
            if nbytes < 0:
                nv.check(int(nbytes), "gs_envmap_scratch_bytes")
            if nbytes > 0:
                scratch = nv.scratch(nbytes, dev)
        nv.check(getattr(nv.lib(), self.bwd_name)(*self.head, *self.weight_args, nv.ptr(self.projection),
                                                  nv.ptr(self.pose), nv.ptr(grad_out), nv.ptr(d_weight),
                                                  nv.ptr(d_env), nv.ptr(scratch), nbytes, nv.stream()), self.bwd_name)
        return d_env, d_weight


class _CompositeEnvironment(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, env, image, image_weight, projection, T_camera_world, camera, dtype):
        ctx.call = _Call(env, image, image_weight, camera, dtype)
        ctx.env_shape = env.shape
        return ctx.call.forward()

    @staticmethod
    @once_differentiable
    @nv.on_tensor_device
    def backward(ctx, grad_out):
        need_env, need_image, need_weight = ctx.needs_input_grad[:3]
        d_env = d_weight = None
        if need_env or need_weight:
            d_env, d_weight = ctx.call.backward(grad_out, need_env, need_weight)
        return (d_env.view(ctx.env_shape) if need_env else None, grad_out if need_image else None,
                d_weight if need_weight else None, None, None, None, None)


def composite_environment(env: torch.Tensor, image: torch.Tensor | None, image_weight: torch.Tensor | None,
                          camera: CameraParams) -> torch.Tensor:
    """`image + (1 - image_weight) * sky`, the sky looked up in `env` (6, R, R, C) by every pixel's view direction
    (module docstring).  `image` (H, W, C) and `image_weight` (H, W) are a render's `image` and `image_weight`
    (`render_gaussians(..., differentiable_weight=True)` for the weight to pass its gradient on), read through their
    strides; both None gives the sky alone.  Gradients reach env, image and image_weight; the camera gets none."""
    dtype = _check("composite_environment", env, image, image_weight, camera)
    return _CompositeEnvironment.apply(env, image, image_weight, camera.projection, camera.T_camera_world, camera,
                                       dtype)


def sample_environment(env: torch.Tensor, camera: CameraParams) -> torch.Tensor:
    """the sky alone as `camera` sees it: composite_environment(env, None, None, camera)"""
    return composite_environment(env, None, None, camera)


def _positive_int(what, name, v):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise ValueError(f"{what}: {name} must be a positive int, got {v!r}")


def environment_directions(R: int, device=None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(6, R, R, 3): the (unnormalised) world direction of every texel centre under the module's convention -- texel
    (f, j, i) has component f // 2 equal to +1 (f even) or -1 (f odd), and (2 i + 1) / R - 1, (2 j + 1) / R - 1 in the
    two other axes in ascending order.  Looking that direction up lands on face f at (v, u) = (j, i) exactly.  Plain
    torch, off the hot path: fill a map with any function of direction."""
    _positive_int("environment_directions", "R", R)
    centre = (2 * torch.arange(R, device=device, dtype=dtype) + 1) / R - 1
    p, q = centre.view(1, R).expand(R, R), centre.view(R, 1).expand(R, R)
    out = torch.empty((6, R, R, 3), device=device, dtype=dtype)
    for face in range(6):
        axis, sign = face // 2, 1.0 - 2.0 * (face % 2)
        others = [k for k in range(3) if k != axis]
        out[face, :, :, axis] = sign
        out[face, :, :, others[0]] = p
        out[face, :, :, others[1]] = q
    return out


def constant_environment(colour, R: int = 1, device=None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(6, R, R, C) map holding `colour` (C values, C in 1 .. 4) on every texel: the constant `background=` of
    render_gaussians as a starting point for a learnable sky"""
    _positive_int("constant_environment", "R", R)
    c = torch.as_tensor(colour, dtype=dtype, device=device).reshape(-1)
    if not 1 <= c.numel() <= MAX_CHANNELS:
        raise ValueError(f"constant_environment: {c.numel()} channels; 1 to {MAX_CHANNELS} are supported")
    return c.expand(6, R, R, c.numel()).contiguous()
