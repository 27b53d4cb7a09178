"""numpy restatement of include/gs_fusion.h, written from the header's text: the per-voxel integration rule operation by
operation (in f32, or in float64 from the same f32 inputs), and the marching-tetrahedra isosurface with the header's orders,
vectorised over voxels and cells.  Also the mesh invariants the tests check on the restatement's and the kernels' output."""
import itertools
import math

import numpy as np

VIEWS_PER_LAUNCH = 16
EDGE_TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMUTATIONS = tuple(itertools.permutations(range(3)))          # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


def _parity(p):
    """+1 for an even permutation of 0..n-1, -1 for an odd one"""
    return -1 if sum(1 for i in range(len(p)) for j in range(i + 1, len(p)) if p[i] > p[j]) % 2 else 1


def world_to_camera(q, t):
    """(q xyzw, t) of T_pointcloud_camera -> the 3x4 world -> camera matrix, in float64, rounded once to f32"""
    q = np.asarray(q, np.float64).reshape(4)
    t = np.asarray(t, np.float64).reshape(3)
    x, y, z, w = q / math.sqrt(float((q * q).sum()))
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R.T, (-R.T @ t)[:, None]], axis=1).astype(np.float32)


def voxel_positions(dims, origin, step, dtype=np.float32):
    """three broadcastable arrays: origin[a] + idx[a] * step[a], a multiply and an add, each rounded in dtype"""
    out = []
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = dims[a]
        idx = np.arange(dims[a]).astype(dtype).reshape(shape)
        out.append(dtype(origin[a]) + idx * dtype(step[a]))
    return out


def integrate(tsdf, weight, colour, views, origin, voxel, trunc, max_weight, min_alpha, near, dtype=np.float32, fragile=None, stats=None):
    """The rule of gs_tsdf_integrate on numpy volumes, in place, every operation rounded in `dtype`.  views: dicts with depth
    (h,w), alpha (h,w) | None, image (h,w,3) | None, fx, fy, cx, cy, m (3,4), all f32.  fragile: a bool volume that collects
    the voxels one of whose decisions lies within the margins of the f32-against-float64 comparison; stats: a list that receives,
    per view, how many voxels left the rule at each of its skips and how many it updated."""
    f = dtype
    px, py, pz = np.broadcast_arrays(*voxel_positions(tsdf.shape, origin, voxel, f))
    trunc, max_weight, min_alpha, near = f(trunc), f(max_weight), f(min_alpha), f(near)
    with np.errstate(all="ignore"):
        for view in views:
            m = np.asarray(view["m"], np.float32).astype(f)
            h, w = view["depth"].shape
            x = ((m[0, 0] * px + m[0, 1] * py) + m[0, 2] * pz) + m[0, 3]
            y = ((m[1, 0] * px + m[1, 1] * py) + m[1, 2] * pz) + m[1, 3]
            z = ((m[2, 0] * px + m[2, 1] * py) + m[2, 2] * pz) + m[2, 3]
            keep = z > near
            u = f(view["fx"]) * (x / z) + f(view["cx"])
            v = f(view["fy"]) * (y / z) + f(view["cy"])
            keep &= (u >= 0) & (u < f(w)) & (v >= 0) & (v < f(h))
            pu = np.where(keep, np.floor(u), 0).astype(np.int64)
            pv = np.where(keep, np.floor(v), 0).astype(np.int64)
            d = view["depth"][pv, pu].astype(f)
            keep &= (d > 0) & np.isfinite(d)
            if view.get("alpha") is not None:
                keep &= view["alpha"][pv, pu].astype(f) >= min_alpha
            sdf = d - z
            if fragile is not None:
                near_pixel_edge = (np.abs(u - np.round(u)) < 1e-3) | (np.abs(v - np.round(v)) < 1e-3)
                fragile |= (np.abs(z - near) < 1e-6) | ((z > near) & near_pixel_edge) | (keep & (np.abs(sdf + trunc) < 1e-5 * trunc))
            if stats is not None:
                front = z > near
                seen = front & (u >= 0) & (u < f(w)) & (v >= 0) & (v < f(h))
                with_depth = seen & (d > 0) & np.isfinite(d)
                stats.append(dict(behind=int((~front).sum()), left=int((front & (u < 0)).sum()), right=int((front & (u >= f(w))).sum()),
                                  above=int((front & (v < 0)).sum()), below=int((front & (v >= f(h))).sum()),
                                  no_depth=int((seen & ~with_depth).sum()), low_alpha=int((with_depth & ~keep).sum()),
                                  at_min_alpha=0 if view.get("alpha") is None else int((keep & (view["alpha"][pv, pu] == min_alpha)).sum()),
                                  far_behind=int((keep & (sdf < -trunc)).sum()), updated=int((keep & ~(sdf < -trunc)).sum())))
            keep &= ~(sdf < -trunc)
            s = np.fmin(f(1), sdf / trunc)
            W = weight.astype(f)
            Wn = W + f(1)
            tsdf[...] = np.where(keep, (W * tsdf + s) / Wn, tsdf)
            if colour is not None and view.get("image") is not None:
                rgb = view["image"][pv, pu].astype(f)
                colour[...] = np.where(keep[..., None], (W[..., None] * colour + rgb) / Wn[..., None], colour)
            weight[...] = np.where(keep, np.fmin(Wn, max_weight), weight)


def new_volume(dims, colour=True, dtype=np.float32):
    return (np.ones(dims, dtype), np.zeros(dims, dtype), np.zeros(tuple(dims) + (3,), dtype) if colour else None)


# ---- the isosurface ------------------------------------------------------------------------------------------------------
def tetrahedron_triangles():
    """{set of inside corners as a 4-bit case: [triangles]}, a triangle three tetrahedron edges (vi, vj), vi < vj, wound for a
    tetrahedron of determinant +1 -- built from the header's two sentences"""
    edge = lambda a, b: (min(a, b), max(a, b))
    table = {}
    for case in range(16):
        inside = [v for v in range(4) if case >> v & 1]
        outside = [v for v in range(4) if not case >> v & 1]
        if len(inside) in (1, 3):
            lone = inside[0] if len(inside) == 1 else outside[0]
            rest = [v for v in range(4) if v != lone]
            p, q, r = rest
            if _parity((lone, p, q, r)) < 0:
                q, r = r, q
            tri = (edge(lone, p), edge(lone, q), edge(lone, r))
            table[case] = [tri if len(inside) == 1 else (tri[0], tri[2], tri[1])]
        elif len(inside) == 2:
            (i1, i2), (o1, o2) = inside, outside
            if _parity((i1, i2, o1, o2)) < 0:
                o1, o2 = o2, o1
            quad = (edge(i1, o1), edge(i1, o2), edge(i2, o2), edge(i2, o1))
            table[case] = [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
        else:
            table[case] = []
    return table


def tetrahedron_corners(perm):
    """the four corners of the tetrahedron of an axis permutation, as offsets from the cell's base corner"""
    a, b, _ = perm
    v1 = [0, 0, 0]
    v1[a] = 1
    v2 = list(v1)
    v2[b] = 1
    return ((0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1))


def _shifted(arr, a, b, c, fill=False):
    """out[i,j,k] = arr[i+a, j+b, k+c], `fill` where that is outside"""
    out = np.full(arr.shape, fill, arr.dtype)
    n = arr.shape
    src = tuple(slice(max(o, 0), n[d] + min(o, 0)) for d, o in enumerate((a, b, c)))
    dst = tuple(slice(max(-o, 0), n[d] + min(-o, 0)) for d, o in enumerate((a, b, c)))
    out[dst] = arr[src]
    return out


def isosurface(values, origin, spacing, level, valid=None, colour=None, flip=False):
    """-> (vertices (V,3) f32, faces (F,3) int32, colours (V,3) f32 | None) by the header's rule"""
    f = np.float32
    values = np.asarray(values, f)
    level = f(level)
    dims = values.shape
    n = values.size
    empty = (np.zeros((0, 3), f), np.zeros((0, 3), np.int32), None if colour is None else np.zeros((0, 3), f))
    if n == 0 or min(dims) < 2:
        return empty
    ok = np.isfinite(values) if valid is None else np.isfinite(values) & (np.asarray(valid) > 0)
    inside = values < level
    cell = np.ones(dims, bool)                      # processed cells, by base corner; False where there is no cell
    for d in itertools.product((0, 1), repeat=3):
        cell &= _shifted(ok, *d)
    exists = np.zeros(dims + (7,), bool)
    for e, d in enumerate(EDGE_TYPES):
        crossing = inside != _shifted(inside, *d)
        contained = np.zeros(dims, bool)
        for o in itertools.product(*[(0,) if d[a] else (0, -1) for a in range(3)]):
            contained |= _shifted(cell, *o)
        exists[..., e] = crossing & contained
    index = (np.cumsum(exists.ravel()) - 1).reshape(exists.shape)          # vertex number of (owner, edge type)
    owner = np.argwhere(exists)                                            # rows (i, j, k, e) in (linear index, type) order
    A = owner[:, :3]
    B = A + np.array(EDGE_TYPES)[owner[:, 3]]
    with np.errstate(all="ignore"):
        a, b = values[tuple(A.T)], values[tuple(B.T)]
        t = (level - a) / (b - a)
        vertices = np.zeros((len(owner), 3), f)
        for axis in range(3):
            pA = f(origin[axis]) + A[:, axis].astype(f) * f(spacing[axis])
            pB = f(origin[axis]) + B[:, axis].astype(f) * f(spacing[axis])
            vertices[:, axis] = pA + t * (pB - pA)
        colours = None
        if colour is not None:
            cA, cB = np.asarray(colour, f)[tuple(A.T)], np.asarray(colour, f)[tuple(B.T)]
            colours = cA + t[:, None] * (cB - cA)
    table = tetrahedron_triangles()
    type_of = {d: e for e, d in enumerate(EDGE_TYPES)}
    base = np.argwhere(cell)                                               # processed cells in linear order
    faces = np.full((len(base), 6, 2, 3), -1, np.int64)
    for tet, perm in enumerate(PERMUTATIONS):
        corners = tetrahedron_corners(perm)
        swap = (_parity(perm) < 0) != bool(flip)
        case = np.zeros(len(base), np.int64)
        for v, c in enumerate(corners):
            case |= inside[tuple((base + c).T)].astype(np.int64) << v
        for value, triangles in table.items():
            rows = np.nonzero(case == value)[0]
            if not len(rows):
                continue
            for slot, tri in enumerate(triangles):
                tri = (tri[0], tri[2], tri[1]) if swap else tri
                for corner, (vi, vj) in enumerate(tri):
                    lower = base[rows] + corners[vi]
                    e = type_of[tuple(np.subtract(corners[vj], corners[vi]))]
                    faces[rows, tet, slot, corner] = index[tuple(lower.T) + (e,)]
    faces = faces.reshape(-1, 3)
    faces = faces[faces[:, 0] >= 0]
    return vertices, faces.astype(np.int32), colours


# ---- invariants of a mesh -------------------------------------------------------------------------------------------------
def directed_edges(faces):
    faces = np.asarray(faces, np.int64)
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def edge_report(faces):
    """-> (closed and oriented: every directed edge once and its reverse once; largest count of one directed edge; largest
    count of one undirected edge; number of undirected edges)"""
    e = directed_edges(faces)
    if not len(e):
        return True, 0, 0, 0
    key = e[:, 0] * (e.max() + 1) + e[:, 1]
    rev = e[:, 1] * (e.max() + 1) + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    closed = bool(counts.max() == 1 and np.array_equal(uniq, np.unique(rev)))
    und = np.sort(e, axis=1)
    _, ucounts = np.unique(und[:, 0] * (e.max() + 1) + und[:, 1], return_counts=True)
    return closed, int(counts.max()), int(ucounts.max()), int(len(ucounts))


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def triangle_areas(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.linalg.norm(np.cross(b - a, c - a), axis=1) / 2.0


def sphere_values(G, centre=(0.47, 0.52, 0.49), radius=0.31):
    """|p - c| - r in f32 on a G^3 grid over the unit cube -> (values, origin, spacing)"""
    h = np.float32(1.0 / (G - 1))
    x, y, z = voxel_positions((G, G, G), (0.0, 0.0, 0.0), (h, h, h))
    c = np.asarray(centre, np.float32)
    values = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - np.float32(radius)
    return values.astype(np.float32), (0.0, 0.0, 0.0), (float(h),) * 3


def check_sphere_mesh(vertices, faces, G, flip, centre=(0.47, 0.52, 0.49), radius=0.31):
    """the invariants of the sphere mesh (tests/test_fusion_ref_host.py, tests/test_gpu_fusion.py); -> (V, F, worst distance, bound)"""
    closed, _, _, n_edges = edge_report(faces)
    assert closed, "not every directed edge occurs once with its reverse once"
    V, F = len(vertices), len(faces)
    assert V - n_edges + F == 2, (V, n_edges, F)
    assert len(np.unique(faces)) == V and faces.min() == 0 and faces.max() == V - 1, "unreferenced vertex"
    assert triangle_areas(vertices, faces).min() > 0.0, "zero-area triangle"
    volume = signed_volume(vertices, faces)
    assert (volume < 0) if flip else (volume > 0), volume
    h = 1.0 / (G - 1)
    bound = 3 * h * h / (8 * (radius - np.sqrt(3) * h))
    worst = float(np.abs(np.linalg.norm(np.asarray(vertices, np.float64) - np.asarray(centre, np.float64), axis=1) - radius).max())
    assert worst <= bound, (worst, bound)
    return V, F, worst, bound


# ---- synthetic views for the integration tests ----------------------------------------------------------------------------
def look_at_pose(eye, target, up=(0.0, -1.0, 0.0)):
    """(q xyzw, t) of T_pointcloud_camera for a camera at `eye` looking along +z at `target`, x to the right and y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, -np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], axis=1)                       # camera axes as columns: camera -> world
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:                                                          # a half turn: the axis from the diagonal
        axis = np.sqrt(np.maximum(0.0, (np.diag(R) + 1) / 2))
        q = np.array([axis[0], axis[1] * np.sign(R[0, 1] or 1), axis[2] * np.sign(R[0, 2] or 1), 0.0])
    return q.astype(np.float32), eye.astype(np.float32)


def synthetic_view(eye, target, h, w, focal, centre, radius, rng, plane_z=None, alpha=True, image=True, specials=True,
                   min_alpha=0.5, principal=None):
    """A view of a sphere (centre, radius) in front of a plane at camera depth plane_z (None: depth 0 where the sphere is
    missed): depth by ray casting through the pixel centres, in float64 rounded to f32.  focal: one number, or (fx, fy);
    principal: (cx, cy), the middle of the image if None; the rays are cast with them.  specials: a few pixels hold 0, a
    negative depth, NaN and +inf; alpha holds values below and exactly at min_alpha besides 1."""
    q, t = look_at_pose(eye, target)
    m = world_to_camera(q, t)
    c = m[:, :3].astype(np.float64) @ np.asarray(centre, np.float64) + m[:, 3]
    pv, pu = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    fx, fy = (focal, focal) if np.ndim(focal) == 0 else focal
    cx, cy = (w / 2.0, h / 2.0) if principal is None else principal
    d = np.stack([(pu - cx) / fx, (pv - cy) / fy, np.ones_like(pu)], -1)
    a, b, k = (d * d).sum(-1), -2 * (d @ c), c @ c - radius * radius
    disc = b * b - 4 * a * k
    with np.errstate(invalid="ignore"):
        s = (-b - np.sqrt(disc)) / (2 * a)
    depth = np.where((disc >= 0) & (s > 0), s, 0.0 if plane_z is None else plane_z).astype(np.float32)
    view = dict(q=q, t=t, m=m, fx=np.float32(fx), fy=np.float32(fy), cx=np.float32(cx), cy=np.float32(cy), alpha=None, image=None)
    if specials:
        flat = depth.reshape(-1)
        where = rng.choice(flat.size, size=max(8, flat.size // 40), replace=False)
        flat[where] = np.resize(np.array([0.0, -1.5, np.nan, np.inf], np.float32), where.size)
    view["depth"] = depth
    if alpha:
        view["alpha"] = rng.choice(np.array([0.3, min_alpha, 1.0, 1.0, 1.0], np.float32), size=(h, w)).astype(np.float32)
    if image:
        view["image"] = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    return view


def ring_of_views(n, dims, origin, voxel, h, w, focal, rng, distance=2.2, **kwargs):
    """n views around the middle of the volume, at `distance` from it, of a sphere a quarter of the shortest side in radius"""
    extent = (np.asarray(dims) - 1) * np.asarray(voxel, np.float64)
    centre = np.asarray(origin, np.float64) + extent / 2
    views = []
    for i in range(n):
        ang = 2 * np.pi * i / max(n, 1) + 0.3
        eye = centre + distance * np.array([np.sin(ang), 0.25 * np.cos(2 * ang), -np.cos(ang)])
        views.append(synthetic_view(eye, centre, h, w, focal, centre, extent.min() / 4 + 0.05, rng, **kwargs))
    return views
