"""Meshes from a scene (include/gs_fusion.h, csrc/k_fusion.hip): depth frames fused into a truncated signed distance volume on
the device, and an indexed triangle mesh extracted from any device volume by marching tetrahedra.

  volume = TSDFVolume(bbox=mixture.bounding_box(scene), voxel=0.02, device="cuda")
  volume.integrate(depth, q, t, camera_info, alpha=alpha, image=image)     # one view, or lists of views in one call
  mesh = volume.extract_mesh()                                              # Mesh: vertices, faces, colours on the device
  mesh.to_ply("scene.ply")

isosurface() is the extractor alone, for any (nx,ny,nz) f32 volume on the device; isosurface_of_density() applies it to
mixture.density_volume().  The conventions -- voxel positions, the per-voxel integration rule, which corner is inside, the order
of vertices and faces -- are the header's.

What touches the host: a pose (q, t of T_pointcloud_camera) and the intrinsics become the view's world -> camera matrix in
float64 on the host, rounded once to f32, so pass them as host values where a synchronisation matters; a box given as a
device tensor is read once when the volume is made; and an extraction reads its two totals (vertices, faces) between the plan
and the emit -- the one synchronisation of an extraction.  No frame and no volume is ever copied to the host.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native

VIEWS_PER_LAUNCH = 16                           # GS_TSDF_VIEWS_PER_LAUNCH
MAX_VOXELS = 2 ** 30                            # GS_FUSION_MAX_VOXELS
MAX_IMAGE_SIZE = 32768                          # GS_FUSION_MAX_IMAGE_SIZE
ISO_BLOCK = 256                                 # GS_ISO_BLOCK
TRUNC_VOXELS = 4.0                              # the default truncation distance, in (largest) voxel steps
DEFAULT_MAX_WEIGHT = 64.0
DEFAULT_MIN_ALPHA = 0.5

_VP, _I32, _I64, _F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


def cell_ws_bytes(n):
    """GS_ISO_CELL_WS_BYTES"""
    return n * 2


def block_ws_bytes(n):
    """GS_ISO_BLOCK_WS_BYTES"""
    return (n + ISO_BLOCK - 1) // ISO_BLOCK * 16


def voxel_ws_bytes(n):
    """GS_ISO_VOXEL_WS_BYTES"""
    return n * 4


class GsTsdfVolume(C.Structure):
    _fields_ = [("tsdf", _VP), ("weight", _VP), ("colour", _VP), ("nx", _I32), ("ny", _I32), ("nz", _I32),
                ("origin", _F32 * 3), ("voxel", _F32 * 3), ("trunc", _F32), ("max_weight", _F32), ("min_alpha", _F32), ("near", _F32)]

    @classmethod
    def of(cls, tsdf, weight, colour, origin, voxel, trunc, max_weight, min_alpha, near):
        nx, ny, nz = tsdf.shape
        return cls(tsdf=_native.ptr(tsdf), weight=_native.ptr(weight), colour=_native.ptr(colour), nx=nx, ny=ny, nz=nz,
                   origin=(_F32 * 3)(*origin), voxel=(_F32 * 3)(*voxel), trunc=trunc, max_weight=max_weight, min_alpha=min_alpha, near=near)


class GsTsdfView(C.Structure):
    _fields_ = [("depth", _VP), ("alpha", _VP), ("image", _VP), ("h", _I32), ("w", _I32), ("fx", _F32), ("fy", _F32), ("cx", _F32),
                ("cy", _F32), ("m", (_F32 * 4) * 3)]

    @classmethod
    def of(cls, depth, alpha, image, intrinsics, m):
        """depth (h,w), alpha (h,w) | None, image (h,w,3) | None on the device; intrinsics (fx, fy, cx, cy); m (3,4) f32 on the host"""
        view = cls(depth=depth.data_ptr(), alpha=_native.ptr(alpha), image=_native.ptr(image), h=depth.shape[0], w=depth.shape[1],
                   fx=intrinsics[0], fy=intrinsics[1], cx=intrinsics[2], cy=intrinsics[3])
        for r in range(3):
            for c in range(4):
                view.m[r][c] = float(m[r, c])
        return view


class GsIsoVolume(C.Structure):
    _fields_ = [("values", _VP), ("valid", _VP), ("colour", _VP), ("nx", _I32), ("ny", _I32), ("nz", _I32), ("origin", _F32 * 3),
                ("spacing", _F32 * 3), ("level", _F32), ("flip", _I32)]

    @classmethod
    def of(cls, values, valid, colour, origin, spacing, level, flip):
        nx, ny, nz = values.shape
        return cls(values=_native.ptr(values), valid=_native.ptr(valid), colour=_native.ptr(colour), nx=nx, ny=ny, nz=nz,
                   origin=(_F32 * 3)(*origin), spacing=(_F32 * 3)(*spacing), level=level, flip=1 if flip else 0)


ARGTYPES = {
    # (ctx, volume, views, n_views, stream)
    "gs_tsdf_integrate": [_VP, C.POINTER(GsTsdfVolume), C.POINTER(GsTsdfView), _I32, _VP],
    # (ctx, volume, cell_ws, block_ws, totals, stream)
    "gs_isosurface_plan": [_VP, C.POINTER(GsIsoVolume), _VP, _VP, _VP, _VP],
    # (ctx, volume, cell_ws, block_ws, voxel_ws, n_vertices, n_faces, vertices, colours, faces, stream)
    "gs_isosurface_emit": [_VP, C.POINTER(GsIsoVolume), _VP, _VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


def _three(v, what):
    """a scalar or three values -> three finite Python floats"""
    a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError(f"{what} must be one or three finite values")
    return [float(x) for x in a]


def _device_f32(t, shape, device, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"meshes are made on the GPU: {what} must be a tensor on a cuda/hip device (there is no CPU path)")
    if t.device != device or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)} on {device}")
    return t


def world_to_camera(q, t):
    """(q xyzw, t) of T_pointcloud_camera -> the (3,4) world -> camera matrix [R^T | -R^T t], R the rotation of q / |q|, in
    float64 on the host, rounded once to f32"""
    q = np.asarray(q.detach().cpu() if isinstance(q, torch.Tensor) else q, np.float64).reshape(-1)
    t = np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, np.float64).reshape(-1)
    if q.size != 4 or t.size != 3:
        raise ValueError("a view's pose is one quaternion (x,y,z,w) and one translation")
    norm = math.sqrt(float((q * q).sum()))
    if not (math.isfinite(norm) and norm > 0.0 and np.isfinite(t).all()):
        raise ValueError("a view's pose must be finite, with a quaternion of norm > 0")
    x, y, z, w = q / norm
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R.T, (-R.T @ t)[:, None]], axis=1).astype(np.float32)


def _intrinsics(camera_info):
    """(fx, fy, cx, cy) as Python floats of the f32 intrinsics.  The integration rule has no place for K[0,1] and K[1,0], which
    the rasteriser that produced the depth honours: a camera that has either is refused."""
    K = camera_info.camera_intrinsics
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, np.float32)
    if K[0, 1] != 0 or K[1, 0] != 0:
        raise ValueError(f"fusion takes fx, fy, cx, cy only: camera_intrinsics has K[0,1] = {float(K[0, 1])}, K[1,0] = {float(K[1, 0])}")
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


@dataclass
class Mesh:
    """An indexed triangle mesh on the device: vertices (V,3) f32, faces (F,3) int32 into them, colours (V,3) f32 or None"""
    vertices: torch.Tensor
    faces: torch.Tensor
    colours: Optional[torch.Tensor] = None

    def to_ply(self, path):
        """binary little-endian PLY: x y z as float, with colours red green blue as uchar -- (uint8)min(max(c * 255, 0), 255), the
        frames' RGB_TRUNC rule, NaN as 0 -- and the faces as `list uchar int vertex_indices`.  Copies the mesh to the host."""
        vertices = self.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
        faces = self.faces.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
        fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
        if self.colours is not None:
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        rows = np.zeros(len(vertices), dtype=fields)
        rows["x"], rows["y"], rows["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
        if self.colours is not None:
            c = self.colours.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
            with np.errstate(invalid="ignore", over="ignore"):
                u8 = np.fmin(np.fmax(c * np.float32(255.0), np.float32(0.0)), np.float32(255.0)).astype(np.uint8)
            rows["red"], rows["green"], rows["blue"] = u8[:, 0], u8[:, 1], u8[:, 2]
        tris = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        tris["n"], tris["v"] = 3, faces
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vertices)}", "property float x", "property float y",
                  "property float z"]
        if self.colours is not None:
            header += ["property uchar red", "property uchar green", "property uchar blue"]
        header += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
        with open(path, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            fh.write(rows.tobytes())
            fh.write(tris.tobytes())


def isosurface(values, origin, spacing, level, valid=None, colour=None, flip=False) -> Mesh:
    """The level-set mesh of a device volume: values (nx,ny,nz) f32, voxel (i,j,k) at origin + (i,j,k) * spacing; valid (same
    shape, a corner counts where it is > 0 and its value finite) and colour (nx,ny,nz,3) optional.  A corner is inside where
    value < level, and triangles face the value >= level side; flip=True reverses them (a density, higher inside, wants it).
    Vertices in (owner voxel, edge type) order, faces in (cell, tetrahedron, triangle) order, nothing duplicated.  The two
    totals are read from the device between the two library calls: one synchronisation."""
    _bind()
    if not isinstance(values, torch.Tensor) or not values.is_cuda:
        raise ValueError("meshes are made on the GPU: values must be a tensor on a cuda/hip device (there is no CPU path)")
    if values.dim() != 3:
        raise ValueError("values must be an (nx,ny,nz) volume")
    device, dims = values.device, tuple(values.shape)
    values = _device_f32(values.detach(), dims, device, "values")
    valid = None if valid is None else _device_f32(valid.detach(), dims, device, "valid")
    colour = None if colour is None else _device_f32(colour.detach(), dims + (3,), device, "colour")
    n = values.numel()
    if n > MAX_VOXELS:
        raise ValueError(f"at most {MAX_VOXELS} voxels per volume")
    origin, spacing = _three(origin, "origin"), _three(spacing, "spacing")
    empty = lambda dtype: torch.zeros((0, 3), dtype=dtype, device=device)
    if n == 0:
        return Mesh(empty(torch.float32), empty(torch.int32), None if colour is None else empty(torch.float32))
    vol = GsIsoVolume.of(values, valid, colour, origin, spacing, float(level), flip)
    ctx = _native.shared_ctx(device)
    cell_ws = torch.empty(cell_ws_bytes(n) // 2, dtype=torch.int16, device=device)
    block_ws = torch.empty(block_ws_bytes(n) // 8, dtype=torch.int64, device=device)
    totals = torch.zeros(2, dtype=torch.int64, device=device)
    _native.call("gs_isosurface_plan", device, ctx, vol, _native.ptr(cell_ws), _native.ptr(block_ws), _native.ptr(totals))
    n_vertices, n_faces = (int(x) for x in totals.cpu())               # the one host read
    if n_vertices > 2 ** 31 - 1 or n_faces > 2 ** 31 - 1:
        raise ValueError(f"the mesh would have {n_vertices} vertices and {n_faces} faces: more than int32 indices reach")
    vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=device)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=device)
    colours = None if colour is None else torch.empty((n_vertices, 3), dtype=torch.float32, device=device)
    voxel_ws = torch.empty(voxel_ws_bytes(n) // 4, dtype=torch.int32, device=device)
    _native.call("gs_isosurface_emit", device, ctx, vol, _native.ptr(cell_ws), _native.ptr(block_ws), _native.ptr(voxel_ws), n_vertices,
                 n_faces, _native.ptr(vertices), _native.ptr(colours), _native.ptr(faces))
    return Mesh(vertices, faces, colours)


def isosurface_of_density(scene, G, level, bbox=None) -> Mesh:
    """The surface density = level of the scene read as a mixture: mixture.density_volume(scene, G, bbox) on its G^3 sample
    grid, faces outwards (flip: the density is higher inside).  The box is read to the host for the grid's origin and spacing."""
    from . import mixture
    with torch.no_grad():
        bbox = mixture.bounding_box(scene) if bbox is None else bbox
        volume = mixture.density_volume(scene, G, bbox).contiguous()
    box = np.asarray(bbox.detach().cpu(), np.float32).astype(np.float64)
    spacing = (box[1] - box[0]) / max(G - 1, 1)
    return isosurface(volume, box[0], spacing, level, flip=True)


class TSDFVolume:
    """A truncated signed distance volume on the device: tsdf (nx,ny,nz) f32 starting at 1, weight starting at 0 and, with
    colour=True, colour (nx,ny,nz,3) starting at 0; voxel (i,j,k) at origin + (i,j,k) * voxel.

    Either bbox ((2,3): the corners) with voxel (dims = ceil(extent / voxel) + 1 per axis) or with dims (voxel = extent /
    (dims - 1)), or origin with dims and voxel.  trunc defaults to TRUNC_VOXELS (4) times the largest voxel step; a view
    updates a voxel whose signed distance along z is >= -trunc, where the view's accumulated alpha (if given) is >= min_alpha
    and its depth finite and > 0, behind z > near; weights saturate at max_weight."""

    def __init__(self, bbox=None, origin=None, dims=None, voxel=None, trunc=None, max_weight=DEFAULT_MAX_WEIGHT,
                 min_alpha=DEFAULT_MIN_ALPHA, near=0.0, colour=True, device="cuda"):
        _bind()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"a TSDFVolume lives on a GPU, got {self.device} (there is no CPU path)")
        if (bbox is None) == (origin is None):
            raise ValueError("give bbox or origin, not both")
        if bbox is not None:
            box = np.asarray(bbox.detach().cpu() if isinstance(bbox, torch.Tensor) else bbox, np.float64).reshape(2, 3)
            if not np.isfinite(box).all() or not (box[1] > box[0]).all():
                raise ValueError("bbox must be finite with bbox[1] > bbox[0] on every axis")
            extent = box[1] - box[0]
            if (dims is None) == (voxel is None):
                raise ValueError("with bbox give dims or voxel, not both")
            if voxel is not None:
                voxel = _three(voxel, "voxel")
                dims = [int(math.ceil(extent[a] / voxel[a])) + 1 for a in range(3)]
            else:
                dims = [int(d) for d in ((dims,) * 3 if np.isscalar(dims) else dims)]
                if min(dims) < 2:
                    raise ValueError("with bbox every dimension must be >= 2")
                voxel = [float(extent[a] / (dims[a] - 1)) for a in range(3)]
            origin = [float(x) for x in box[0]]
        else:
            if dims is None or voxel is None:
                raise ValueError("with origin give dims and voxel")
            origin, voxel = _three(origin, "origin"), _three(voxel, "voxel")
            dims = [int(d) for d in ((dims,) * 3 if np.isscalar(dims) else dims)]
        if len(dims) != 3 or min(dims) < 0 or dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            raise ValueError(f"dims must be three sizes >= 0 with at most {MAX_VOXELS} voxels, got {dims}")
        if not all(v > 0 for v in voxel):
            raise ValueError("voxel must be > 0")
        self.dims, self.origin, self.voxel = tuple(dims), origin, voxel
        self.trunc = float(TRUNC_VOXELS * max(voxel) if trunc is None else trunc)
        self.max_weight, self.min_alpha, self.near = float(max_weight), float(min_alpha), float(near)
        if not (self.trunc > 0 and math.isfinite(self.trunc) and self.max_weight > 0 and math.isfinite(self.max_weight)):
            raise ValueError("trunc and max_weight must be finite and > 0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tsdf = torch.ones(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.colour = torch.zeros(self.dims + (3,), dtype=torch.float32, device=self.device) if colour else None

    def _view(self, depth, q, t, camera_info, alpha, image, keep):
        depth = _device_f32(depth.detach() if isinstance(depth, torch.Tensor) else depth, getattr(depth, "shape", ()), self.device, "depth")
        if depth.dim() != 2 or max(depth.shape) > MAX_IMAGE_SIZE:
            raise ValueError(f"depth must be (h,w) with h, w <= {MAX_IMAGE_SIZE}")
        h, w = depth.shape
        if (camera_info.camera_height, camera_info.camera_width) != (h, w):
            raise ValueError(f"the frame is {h}x{w}, its camera {camera_info.camera_height}x{camera_info.camera_width}")
        alpha = None if alpha is None else _device_f32(alpha.detach(), (h, w), self.device, "alpha")
        image = None if image is None else _device_f32(image.detach(), (h, w, 3), self.device, "image")
        keep += [depth, alpha, image]
        return GsTsdfView.of(depth, alpha, image, _intrinsics(camera_info), world_to_camera(q, t))

    def integrate(self, depth, q, t, camera_info, alpha=None, image=None):
        """Fuse one view -- depth (h,w) f32 on the device, the rasteriser's depth; q (x,y,z,w), t of T_pointcloud_camera;
        camera_info with the intrinsics and (h,w); optionally the accumulated alpha (h,w) and the image (h,w,3) -- or, with
        lists (tuples) of the same length for depth, q, t and (where given) alpha and image and one camera_info or a list,
        all of them in order in ONE library call (launches of VIEWS_PER_LAUNCH views).  Queued on the current stream."""
        if isinstance(depth, (list, tuple)):
            n = len(depth)
            cameras = list(camera_info) if isinstance(camera_info, (list, tuple)) else [camera_info] * n
            alphas, images = ([None] * n if x is None else list(x) for x in (alpha, image))
            if not (len(q) == len(t) == len(cameras) == len(alphas) == len(images) == n):
                raise ValueError("q, t, and where given as sequences camera_info, alpha and image must have one entry per depth frame")
            args = [(depth[i], q[i], t[i], cameras[i], alphas[i], images[i]) for i in range(n)]
        else:
            args = [(depth, q, t, camera_info, alpha, image)]
        if not args:
            return self
        keep = []
        views = (GsTsdfView * len(args))(*[self._view(*a, keep) for a in args])
        vol = GsTsdfVolume.of(self.tsdf, self.weight, self.colour, self.origin, self.voxel, self.trunc, self.max_weight, self.min_alpha, self.near)
        _native.call("gs_tsdf_integrate", self.device, _native.shared_ctx(self.device), vol, views, len(args))
        return self

    def extract_mesh(self, level=0.0, flip=False) -> Mesh:
        """The surface tsdf = level over the voxels a view has reached (weight > 0), coloured if the volume is; faces look
        towards the free side (tsdf >= level) unless flip.  One synchronisation (isosurface)."""
        return isosurface(self.tsdf, self.origin, self.voxel, level, valid=self.weight, colour=self.colour, flip=flip)

