/* gs_fusion.h -- a surface from a trained scene: rendered depth frames fused into a truncated signed distance volume on the
 * device, and an indexed triangle mesh extracted from any device volume (a TSDF, or mixture.density_volume's density).
 *
 *   gs_tsdf_integrate(ctx, &volume, views, n_views, stream);                      // any number of times
 *   gs_isosurface_plan(ctx, &iso, cell_ws, block_ws, totals, stream);            // totals: int64[2] on the device
 *   ... the caller reads totals = {V, F} (the one host read), allocates ...
 *   gs_isosurface_emit(ctx, &iso, cell_ws, block_ws, voxel_ws, V, F, vertices, colours, faces, stream);
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error(), the call's stream last.  Not part of
 * GS_ABI_VERSION's function list.  No call synchronises with the host or allocates; nothing here uses an atomic or a float
 * reduction, so every output is bit-reproducible.  Every f32 operation below is rounded on its own (no contraction).
 *
 * ---- volumes ----
 * A volume is (nx,ny,nz) f32, contiguous, z fastest (voxel (i,j,k) at (i * ny + j) * nz + k: its linear index); a colour
 * volume is (nx,ny,nz,3).  Voxel (i,j,k) sits at origin[a] + (float)idx[a] * step[a] per axis a: one multiply, one add.
 * A new TSDF volume is tsdf = 1, weight = 0, colour = 0.
 *
 * ---- gs_tsdf_integrate: per voxel, the views strictly in order ----
 *   x = ((m[0][0]*px + m[0][1]*py) + m[0][2]*pz) + m[0][3]     (y from row 1, z from row 2: world -> camera)
 *   skip unless z > near
 *   u = fx * (x / z) + cx;  v = fy * (y / z) + cy
 *   skip unless 0 <= u < (float)w and 0 <= v < (float)h        (float comparisons before any conversion: NaN skips)
 *   pu = (int)floorf(u);  pv = (int)floorf(v)                  (pixel pu covers [pu, pu + 1): pixel centres at +0.5)
 *   d = depth[pv * w + pu];  skip unless d > 0 and d is finite
 *   skip if alpha is given and not (alpha[pv * w + pu] >= min_alpha)
 *   sdf = d - z;  skip if sdf < -trunc
 *   s = fminf(1, sdf / trunc)
 *   W = weight;  Wn = W + 1
 *   tsdf = (W * tsdf + s) / Wn
 *   colour[c] = (W * colour[c] + image[(pv * w + pu) * 3 + c]) / Wn      (only with both the volume's colour and the view's image)
 *   weight = fminf(Wn, max_weight)
 * depth is the rasteriser's D = sum w_i d_i / max(A, 1e-6) with d_i the camera-space z: the distance is projective along z;
 * alpha is its accumulated alpha A.
 * How (csrc/k_fusion.hip): a thread owns a voxel, lanes run along z; a launch walks up to GS_TSDF_VIEWS_PER_LAUNCH views
 * whose structs travel in the kernel arguments (the view loop is wave-uniform) and reads and writes each voxel once; a call
 * with more views is cut into consecutive launches, in order.
 *
 * ---- the isosurface: marching tetrahedra on the Kuhn split of every cell ----
 *  - A corner is VALID iff its value is finite and (valid is NULL or valid > 0); it is INSIDE iff value < level.
 *  - The cell with base corner b = (i,j,k), i < nx-1, j < ny-1, k < nz-1, is PROCESSED iff its 8 corners are valid.  Its linear
 *    index is b's.
 *  - It is split into six tetrahedra, one per permutation (a,b',c) of the axes, in lexicographic order
 *    0 xyz, 1 xzy, 2 yxz, 3 yzx, 4 zxy, 5 zyx:  v0 = b, v1 = v0 + e_a, v2 = v1 + e_b', v3 = b + (1,1,1).
 *    Tetrahedra 0, 3, 4 (even permutations) have det[v1-v0, v2-v0, v3-v0] = +1, the others -1.
 *  - Every edge of a tetrahedron runs from a lower corner A to A + (dx,dy,dz), d in {0,1}^3 \ 0, and is OWNED by A's voxel as
 *    edge type 0 +x, 1 +y, 2 +z, 3 +x+y, 4 +x+z, 5 +y+z, 6 +x+y+z.
 *  - A mesh vertex exists iff the ends of its edge differ in INSIDE and at least one processed cell contains the edge (an axis
 *    edge lies in up to four cells, a face diagonal in up to two, the body diagonal in one).  With a = value(A), b = value(B):
 *       t = (level - a) / (b - a);   p[axis] = pA + t * (pB - pA);   colour[c] = cA + t * (cB - cA)
 *    Vertices are ordered by (owner's linear index, edge type).
 *  - Triangles of a tetrahedron, by the set of its inside corners.  Name the crossing on edge (vi,vj) Eij.
 *      one corner l inside, or one corner l outside: with (l,p,q,r) the even permutation of (0,1,2,3) that starts with l and
 *        has p the smallest of the others -- (0,1,2,3), (1,0,3,2), (2,0,1,3), (3,0,2,1) -- the triangle (Elp, Elq, Elr) when l
 *        is inside, (Elp, Elr, Elq) when l is outside;
 *      two inside, i1 < i2, and two outside o1 < o2, swapped if (i1,i2,o1,o2) is an odd permutation: the quad
 *        (Ei1o1, Ei1o2, Ei2o2, Ei2o1) as triangle 0 = (Ei1o1, Ei1o2, Ei2o2) and triangle 1 = (Ei1o1, Ei2o2, Ei2o1): the fixed
 *        diagonal joins Ei1o1 and Ei2o2.
 *    That is the winding for a tetrahedron of determinant +1: the right-hand normal points to the value >= level side.  In a
 *    tetrahedron of determinant -1 the last two indices of every triangle are exchanged; flip != 0 exchanges them once more
 *    (a density volume, higher inside, wants flip).
 *  - Triangles are ordered by (cell's linear index, tetrahedron 0..5, triangle 0..1).  Faces are int32 indices into the vertex
 *    array; no vertex is duplicated and none is unreferenced.
 * How: gs_isosurface_plan records per voxel the mask of its owned crossings and its cell's triangle count (one pass, one
 * 16-bit word per voxel), the per-block sums (GS_ISO_BLOCK voxels per block), their exclusive prefix sums over the volume and
 * the two totals.  gs_isosurface_emit finishes the prefix sums per voxel, writes the vertices, then the faces, which find a
 * vertex as (its owner's first vertex) + (the owner's crossings of lower type): no hashing.
 */
#ifndef GS_FUSION_H
#define GS_FUSION_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_TSDF_VIEWS_PER_LAUNCH 16
#define GS_FUSION_MAX_VOXELS 1073741824            /* 2^30 = 1024^3 */
#define GS_FUSION_MAX_IMAGE_SIZE 32768
#define GS_ISO_BLOCK 256                           /* voxels per block of the plan's and the emit's scans */
/* bytes of the caller's work buffers for a volume of n voxels (n > 0) */
#define GS_ISO_CELL_WS_BYTES(n) ((int64_t)(n) * 2)
#define GS_ISO_BLOCK_WS_BYTES(n) ((((int64_t)(n) + GS_ISO_BLOCK - 1) / GS_ISO_BLOCK) * 16)
#define GS_ISO_VOXEL_WS_BYTES(n) ((int64_t)(n) * 4)

typedef struct gs_tsdf_volume {
    float* tsdf;            /* (nx,ny,nz) */
    float* weight;          /* (nx,ny,nz) */
    float* colour;          /* (nx,ny,nz,3) or NULL */
    int32_t nx, ny, nz;
    float origin[3];
    float voxel[3];         /* the step per axis */
    float trunc;
    float max_weight;
    float min_alpha;
    float near;
} gs_tsdf_volume;

typedef struct gs_tsdf_view {
    const float* depth;     /* (h,w) */
    const float* alpha;     /* (h,w) or NULL */
    const float* image;     /* (h,w,3) or NULL */
    int32_t h, w;
    float fx, fy, cx, cy;
    float m[3][4];          /* world -> camera */
} gs_tsdf_view;

typedef struct gs_iso_volume {
    const float* values;    /* (nx,ny,nz) */
    const float* valid;     /* (nx,ny,nz) or NULL */
    const float* colour;    /* (nx,ny,nz,3) or NULL */
    int32_t nx, ny, nz;
    float origin[3];
    float spacing[3];
    float level;
    int32_t flip;
} gs_iso_volume;

/* volume: a host struct of device pointers; views: a host array of n_views structs of device pointers.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx, volume or (n_views > 0) views NULL; a dimension or n_views
 * negative; nx ny nz above GS_FUSION_MAX_VOXELS; a voxel step, trunc or max_weight not > 0 or not finite; origin, min_alpha or
 * near not finite; with a non-empty volume NULL tsdf or weight; a view with NULL depth, h or w outside
 * [0, GS_FUSION_MAX_IMAGE_SIZE] or a non-finite fx, fy, cx, cy or m.  An empty volume or n_views == 0 is GS_OK with no launch. */
int gs_tsdf_integrate(gs_ctx* ctx, const gs_tsdf_volume* volume, const gs_tsdf_view* views, int32_t n_views, gs_stream stream);

/* cell_ws, block_ws: device work buffers of GS_ISO_CELL_WS_BYTES(n), GS_ISO_BLOCK_WS_BYTES(n) bytes (8-byte aligned), n = nx ny nz,
 * which gs_isosurface_emit reads; totals: int64[2] in device memory, receives {vertices, faces}.
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx or volume NULL; a dimension negative; n above
 * GS_FUSION_MAX_VOXELS; a spacing not > 0 or not finite; origin or level not finite; with n > 0: NULL values, cell_ws, block_ws
 * or totals.  n == 0 is GS_OK with no launch and totals untouched (the mesh is empty). */
int gs_isosurface_plan(gs_ctx* ctx, const gs_iso_volume* volume, void* cell_ws, void* block_ws, int64_t* totals, gs_stream stream);

/* After gs_isosurface_plan on the same volume and buffers, with the totals it wrote.  voxel_ws: GS_ISO_VOXEL_WS_BYTES(n) bytes
 * of device memory (4-byte aligned); vertices (n_vertices,3) f32; colours (n_vertices,3) f32 or NULL (written only with the
 * volume's colour); faces (n_faces,3) int32.  No store goes beyond the counts given.
 * GS_ERR_INVALID_ARGUMENT as for the plan, and: n_vertices or n_faces negative or above 2^31 - 1; NULL voxel_ws; NULL vertices
 * with n_vertices > 0; NULL faces with n_faces > 0.  n == 0, or both counts 0, is GS_OK with no launch. */
int gs_isosurface_emit(gs_ctx* ctx, const gs_iso_volume* volume, const void* cell_ws, const void* block_ws, void* voxel_ws,
                       int64_t n_vertices, int64_t n_faces, float* vertices, float* colours, int32_t* faces, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
