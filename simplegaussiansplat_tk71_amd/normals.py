"""Normals on the HIP library (csrc/gcp_normal.hip): the per-Gaussian normals a camera's list is blended with
(`gaussian_normals` -> `cuda_kernel.render(normal=)`), and 2DGS's depth-normal consistency loss on the rendered maps
(`normal_consistency`, one kernel per direction).  The float64 PyTorch statements both are tested against:
tests/normal_torch.py.  GPU tensors only."""
import torch

from . import _lib

ALPHA_MIN = 1e-3


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, variance_q, variance_scale, mean, P_c, index):
        if not variance_q.is_cuda:
            raise RuntimeError("gaussian_normals is a HIP kernel: tensors must live on the GPU (no CPU path)")
        dev, n = variance_q.device, variance_q.shape[0]
        q, ls, mu, P = (t.detach().contiguous().float() for t in (variance_q, variance_scale, mean, P_c))
        if tuple(q.shape) != (n, 4) or tuple(ls.shape) != (n, 3) or tuple(mu.shape) != (n, 3) or tuple(P.shape) != (3, 4):
            raise RuntimeError("gaussian_normals expects variance_q (N, 4), variance_scale (N, 3), mean (N, 3) and P_c (3, 4)")
        idx = index.detach().contiguous()
        if idx.dtype != torch.int64 or idx.dim() != 1 or any(t.device != dev for t in (ls, mu, P, idx)):
            raise RuntimeError("gaussian_normals expects an int64 (m,) index and every tensor on one device")
        m = idx.shape[0]
        normal = torch.empty(m, 3, dtype=torch.float32, device=dev)
        aux = torch.empty(m, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gcp_normals_forward(q.data_ptr(), ls.data_ptr(), mu.data_ptr(), P.data_ptr(), idx.data_ptr(), n, m,
                                                       normal.data_ptr(), aux.data_ptr(), _stream(dev)), "gcp_normals_forward")
        ctx.save_for_backward(q, P, idx, aux)
        ctx.dtype = variance_q.dtype
        return normal

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_normal):
        q, P, idx, aux = ctx.saved_tensors
        g = g_normal.contiguous().float()
        g_q = torch.empty_like(q)  # every row is written
        with torch.cuda.device(q.device):
            _lib.check(_lib.load().gcp_normals_backward(q.data_ptr(), P.data_ptr(), idx.data_ptr(), aux.data_ptr(), g.data_ptr(), q.shape[0],
                                                        idx.shape[0], g_q.data_ptr(), _stream(q.device)), "gcp_normals_backward")
        return g_q.to(ctx.dtype), None, None, None, None


def gaussian_normals(variance_q, variance_scale, mean, P_c, index):
    """The normals of one camera's list -> float32 (m, 3) in list order, for `cuda_kernel.render(normal=)`.
    variance_q (N, 4 xyzw), variance_scale (N, 3, the raw log scale), mean (N, 3), P_c (3, 4) world->camera with a rotation in
    its left block (as COLMAP poses are), index int64 (m,): the camera's list (`camera_inputs`' "index"; no repeats; m = N with
    the culled entries of a capture-safe list is fine).  For entry j, i = index[j]: the column of R(q_i / max(|q_i|, 1e-8)) that
    belongs to the smallest log scale (ties: the lowest axis) — the axis the Gaussian is flattest along, the same under the 3-D
    filter, which adds one phi^2 to all three — rotated into the camera and negated where it points away from it
    (n . t_c <= 0 afterwards, t_c the centre in camera coordinates).  Differentiable in variance_q only, through the column and
    the normalisation; the axis choice and the flip are piecewise constant, so variance_scale and mean get None.  One HIP launch
    per direction (csrc/gcp_normal.hip), no atomics, nothing read back (capturable); GPU tensors only."""
    return _GaussianNormals.apply(variance_q, variance_scale, mean, P_c, index)


def _maps(what, depth, alpha, normal, K):
    """The refusals, before the library is touched -> (D, A, N, K): contiguous float32, detached."""
    if not (torch.is_tensor(depth) and depth.dim() == 4 and depth.shape[1] == 1 and alpha.shape == depth.shape):
        raise RuntimeError(f"{what} expects depth and alpha of one shape (B, 1, H, W)")
    b, _, h, w = depth.shape
    if tuple(normal.shape) != (b, 3, h, w) or tuple(K.shape) != (b, 3, 3):
        raise RuntimeError(f"{what} expects normal (B, 3, H, W) and K (B, 3, 3) with B, H, W = {b}, {h}, {w}")
    if not depth.is_cuda:
        raise RuntimeError(f"{what} is a HIP kernel: tensors must live on the GPU (no CPU path)")
    if any(t.device != depth.device for t in (alpha, normal, K)):
        raise RuntimeError(f"{what}: depth, alpha, normal and K must live on one device (K too: it is read by the kernel)")
    return tuple(t.detach().contiguous().float() for t in (depth, alpha, normal, K))


def _forward(D, A, N, K, alpha_min, want_e=False, want_n=False):
    """-> (the mean of e as a float64 scalar on the device, e_map or None, depth normals or None)"""
    b, _, h, w = D.shape
    lib = _lib.load()
    dev = D.device
    e_map = torch.empty_like(D) if want_e else None
    dn = torch.empty_like(N) if want_n else None
    with torch.cuda.device(dev):
        partial = torch.empty(lib.gcp_normal_consistency_blocks(b, h, w), dtype=torch.float32, device=dev)
        _lib.check(lib.gcp_normal_consistency_forward(D.data_ptr(), A.data_ptr(), N.data_ptr(), K.data_ptr(), b, h, w, float(alpha_min),
                                                      e_map.data_ptr() if want_e else None, dn.data_ptr() if want_n else None,
                                                      partial.data_ptr(), _stream(dev)), "gcp_normal_consistency_forward")
    return partial.double().sum() / D.numel(), e_map, dn


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, normal, K, alpha_min):
        D, A, N, Kd = _maps("normal_consistency", depth, alpha, normal, K)
        mean, _, _ = _forward(D, A, N, Kd, alpha_min)
        ctx.save_for_backward(D, A, N, Kd)
        ctx.alpha_min, ctx.dtypes = alpha_min, (depth.dtype, alpha.dtype, normal.dtype)
        return mean.to(depth.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        D, A, N, Kd = ctx.saved_tensors
        b, _, h, w = D.shape
        # dLoss / d(sum of e): the quotient is formed in float64 and rounded once, so that an image's gradients under an upstream
        # B in a batch of B are the bits of that image alone under an upstream 1
        scale = (grad_out.reshape(1).double() / D.numel()).float().contiguous()
        g_D, g_A, g_N = torch.empty_like(D), torch.empty_like(A), torch.empty_like(N)  # every word is written
        with torch.cuda.device(D.device):
            _lib.check(_lib.load().gcp_normal_consistency_backward(D.data_ptr(), A.data_ptr(), N.data_ptr(), Kd.data_ptr(), b, h, w,
                                                                   float(ctx.alpha_min), scale.data_ptr(), g_D.data_ptr(), g_A.data_ptr(),
                                                                   g_N.data_ptr(), _stream(D.device)), "gcp_normal_consistency_backward")
        return (*(g.to(t) for g, t in zip((g_D, g_A, g_N), ctx.dtypes)), None, None)


def normal_consistency(depth, alpha, normal, K, alpha_min=ALPHA_MIN):
    """2DGS's normal-consistency loss of rendered maps -> a scalar, differentiable in depth, alpha and normal.
    depth (B, 1, H, W) and alpha (B, 1, H, W): `GS_model_with_param.render`'s maps (depth NOT divided by alpha), normal
    (B, 3, H, W): its normal map (`render(normals=True)`: sum_k w_k n_k in camera coordinates, not divided by alpha either),
    K (B, 3, 3) on the device: the cameras the maps were rendered with (the kernel reads it; nothing goes through the host).
    Per image and pixel p = (x, y):  z = depth / alpha where valid (alpha >= alpha_min and depth > 0);  pt = z r with
    r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) — pixel centres at +0.5 in K's coordinates, as the projection documents;
    n~ = c / |c|, c = (pt(x, y+1) - pt(x, y-1)) x (pt(x+1, y) - pt(x-1, y)) where p and its four neighbours are inside the frame
    and valid (2DGS's depth_to_normal; a fronto-parallel surface gives (0, 0, -1), towards the camera; |c| > 0 there, so the
    normalisation needs no epsilon);  e = 1 - a normal . n~ with a = alpha(p) held constant (2DGS's alpha.detach(): no gradient
    through that factor), e = 1 elsewhere (2DGS's zero border).  The loss is the mean of e over all B H W pixels.
    `alpha_min` (default 1e-3) only guards the division depth / alpha: a faint pixel's term is already weighted by
    a |normal| <= alpha^2.  It is not tuned.
    One HIP kernel per direction (csrc/gcp_normal.hip: a 32 x 16 tile and its halo in LDS; the backward is a gather over the
    13-pixel footprint and saves nothing), per-tile sums added in float64, no atomics: two calls give the same bits, and an
    image's e and gradients depend on that image alone.  The upstream gradient is read on the device: capturable.
    GPU tensors only."""
    return _NormalConsistency.apply(depth, alpha, normal, K, float(alpha_min))


def median_as_depth(median, alpha):
    """The median depth map of `render(median=True)` as the pair `normal_consistency`, `depth_normals` and
    `TSDFVolume.integrate` take — "(depth NOT divided by alpha, alpha)" -> (median * alpha.detach(), alpha.detach()).  Those
    kernels stay as they are and recover the median by their own division.  No gradient reaches alpha through either: the
    median depth does not depend on alpha, and the product only undoes the consumers' division."""
    a = alpha.detach()
    return median * a, a


@torch.no_grad()
def normal_consistency_map(depth, alpha, normal, K, alpha_min=ALPHA_MIN):
    """The per-pixel term of `normal_consistency` -> (e float32 (B, 1, H, W), defined bool (B, 1, H, W)), detached: e = 1 where
    `defined` is False.  The same kernel with its two optional outputs."""
    D, A, N, Kd = _maps("normal_consistency_map", depth, alpha, normal, K)
    _, e_map, dn = _forward(D, A, N, Kd, alpha_min, want_e=True, want_n=True)
    return e_map, (dn != 0).any(dim=1, keepdim=True)


@torch.no_grad()
def depth_normals(depth, alpha, K, alpha_min=ALPHA_MIN):
    """The normals of the rendered depth surface, n~ of `normal_consistency` -> float32 (B, 3, H, W) unit vectors in camera
    coordinates, exactly 0 where not defined; detached.  For viewing and for tests."""
    if not (torch.is_tensor(depth) and depth.dim() == 4):
        raise RuntimeError("depth_normals expects depth and alpha of one shape (B, 1, H, W)")
    b, _, h, w = depth.shape
    D, A, N, Kd = _maps("depth_normals", depth, alpha, depth.new_zeros(b, 3, h, w), K)
    return _forward(D, A, N, Kd, alpha_min, want_n=True)[2]
