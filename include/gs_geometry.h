/* gs_geometry.h -- geometry regularisers on the rasteriser's depth output: the camera-space normal of the rendered surface, a
 * cosine loss of that normal against a normal prior, and an edge-aware smoothness of the depth, each loss with its gradient.
 *
 *   gs_depth_normals        (ctx, D, H, W, fx, fy, cx, cy, max_rel_jump, normals, stream);                     // normals (3,H,W)
 *   gs_normal_loss_forward  (ctx, D, N, w_n, w_p_or_NULL, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms, stream);
 *   gs_normal_loss_backward (ctx, D, N, w_n, w_p_or_NULL, H, W, fx, fy, cx, cy, max_rel_jump, flags, terms, upstream_or_NULL, grad_D, stream);
 *   gs_depth_smooth_forward (ctx, D, I_or_NULL, w_p_or_NULL, H, W, edge_lambda, flags, terms, stream);
 *   gs_depth_smooth_backward(ctx, D, I_or_NULL, w_p_or_NULL, H, W, edge_lambda, flags, terms, upstream_or_NULL, grad_D, stream);
 *
 * Same library, same rules as gs_depth.h: status codes, gs_last_error(), the call's stream last.  Not part of GS_ABI_VERSION's
 * function list.  No call synchronises with the host or allocates caller-visible memory; the host never reads the data.  No
 * float atomic anywhere: the same inputs give the same bits on every run.  Every f64 operation below is rounded on its own (no
 * contraction), in the order the parentheses give; division and square root are correctly rounded; exp (float64) is the one
 * operation that is not.  (csrc/k_geometry.hip)
 *
 * ---- common rules ----
 * All planes are contiguous f32 on the device; pixel (x, y) of an (H, W) plane is element p = y W + x, plane k of a (3,H,W)
 * image begins k H W floats behind plane 0.  A depth is VALID iff D > 0 && D <= FLT_MAX (an empty pixel renders 0 and is not
 * valid).  A weight plane enters as a = w > 0 ? w : 0 (a negative or NaN weight is 0); a NULL weight plane counts as 1; a
 * product of weights is one f32 multiply per factor, left to right.  Past the loads and that product everything is float64 on
 * the f32 inputs (the passes are bound by memory), and a result is rounded once to f32.  Selection, not multiplication: a pixel,
 * pair or triple that is not selected adds nothing to any sum, whatever it holds (NaN, inf), and what only unselected terms
 * reach is exactly +0.  fx, fy, cx, cy are the pinhole intrinsics, pixel centres at +0.5; the camera frame is the rasteriser's:
 * x right, y down, z forward.
 *
 * ---- the normal at (x, y) ----
 *   a_x = ((double)x + 0.5 - cx) / fx,   b_y = ((double)y + 0.5 - cy) / fy
 *   with l = D(x-1,y), r = D(x+1,y), u = D(x,y-1), d = D(x,y+1), m = D(x,y), dx = r - l, dy = d - u:
 *   Px = (a_{x+1} r - a_{x-1} l,  b_y dx,  dx)           the back-projected points P = (a D, b D, D), central differences
 *   Py = (a_x dy,  b_{y+1} d - b_{y-1} u,  dy)
 *   c  = Py x Px = (Py.y Px.z - Py.z Px.y,  Py.z Px.x - Py.x Px.z,  Py.x Px.y - Py.y Px.x)
 *   q  = (c.x c.x + c.y c.y) + c.z c.z,   len = sqrt(q),   n = (c.x / len, c.y / len, c.z / len)
 * A fronto-parallel plane gives (0, 0, -1): towards the camera.  The normal EXISTS iff 1 <= x <= W - 2 and 1 <= y <= H - 2; l, r,
 * u, d and m are valid; with max_rel_jump > 0 also |dx| <= max_rel_jump m and |dy| <= max_rel_jump m (a normal is never taken
 * across a depth edge; 0 switches the test off); and q > 0 && q <= DBL_MAX.  The normal does not depend on m but through these
 * selections.  gs_depth_normals writes n rounded to f32 into the three planes, and +0 into all three where it does not exist.
 *
 * ---- gs_normal_loss_forward / gs_normal_loss_backward ----
 *   prior      v = (double)N_k(p); with GS_GEOM_PRIOR_UNIT_RANGE m_k = 2 v - 1 (an 8-bit normal image resampled to [0, 1]), else
 *              m_k = v; with GS_GEOM_PRIOR_FLIP_YZ m_y and m_z are negated (a prior in the OpenGL camera frame: y up, z towards
 *              the viewer).  k = sqrt((m_x m_x + m_y m_y) + m_z m_z).  The prior is USABLE iff k >= 0.5 && k <= DBL_MAX, and
 *              then h = m / k.  (A resampled mix of opposing normals shortens: such a pixel is left out, not normalised.)
 *   selection  w = a(w_n) * a(w_p).  Pixel p is SELECTED iff its normal exists, its prior is usable and w > 0.
 *   loss       cos = (n.x h.x + n.y h.y) + n.z h.z.   L = (sum w (1 - cos)) / (sum w) =: S_l / S_w.
 *   terms      8 floats of device memory, written: { L, S_w, number selected, (sum cos) / number selected, 0, 0, 0, 0 }, each
 *              a float64 value rounded once.  Nothing selected: eight zeros, every gradient +0, nothing NaN.
 *   backward   reads terms[1] (the f32 S_w) on the device and selects anew.  With t = *upstream (NULL: 1) and s = t / S_w, the
 *              normal at a selected pixel has
 *                  g  = -(s w) (h - cos n) / len              dL/dc, through the normalisation
 *                  gx = g x Py,   gy = Px x g                 dL/dPx, dL/dPy, through the cross product
 *              and OWES its four neighbours, through the differences and the back-projection,
 *                  right  (gx.x a_{x+1} + gx.y b_y) + gx.z         left  -((gx.x a_{x-1} + gx.y b_y) + gx.z)
 *                  down   (gy.x a_x + gy.y b_{y+1}) + gy.z         up    -((gy.x a_x + gy.y b_{y-1}) + gy.z)
 *              The backward is a GATHER: grad_D(p) starts at +0 and takes, in this order, what the normal at the left
 *              neighbour owes its right, the right neighbour its left, the upper neighbour its down, the lower neighbour its
 *              up; each of those normals is formed from its own neighbours (once per block, for the tile grown by one pixel on
 *              every side, and kept in LDS as float64), and one that is not selected adds nothing.
 *              This is the exact derivative of L in D with the selections (the jump test among them) held fixed.  Every
 *              element of grad_D is written.
 *
 * ---- gs_depth_smooth_forward / gs_depth_smooth_backward ----
 *   space      x = 1 / D with GS_GEOM_INVERSE, else x = D.
 *   guide      I is a planar (3,H,W) image or NULL.  For two pixels i, j:  e(i, j) = exp(-(edge_lambda * t)) with
 *              t = ((|I_r(j) - I_r(i)| + |I_g(j) - I_g(i)|) + |I_b(j) - I_b(i)|) / 3; without a guide e = 1.  !(t <= DBL_MAX)
 *              unselects the term.
 *   first order (default)  terms are the pairs (p, p + 1) inside a row and (p, p + W) inside a column.  A pair (i, j) is SELECTED
 *              iff both depths are valid, w = a(w_p(i)) * a(w_p(j)) > 0, and the guide allows it; r = x(j) - x(i), v = |r|.
 *   GS_GEOM_SECOND_ORDER   terms are the triples (p - 1, p, p + 1) inside a row and (p - W, p, p + W) inside a column.  A triple
 *              (i, c, j) is SELECTED iff the three depths are valid, w = (a(i) * a(c)) * a(j) > 0, and the guide of the outer
 *              pair e(i, j) allows it; r = (x(i) - 2 x(c)) + x(j), v = |r|.  A depth that is affine in the pixel coordinates costs
 *              nothing in depth space; the depth of a slanted plane seen through a pinhole is affine in INVERSE depth, and costs
 *              nothing there.
 *   loss       L = (sum (w e) v) / (sum w) over the selected terms of both directions.  Pixel p owns the terms that begin
 *              (first order) or are centred (second order) at p, the horizontal one first.
 *   terms      { L, S_w, number of selected terms, 0, 0, 0, 0, 0 }; nothing selected: eight zeros and a gradient of +0.
 *   backward   with s = t / S_w as above and sg(r) = (r > 0) - (r < 0) (0 at 0), the gather at p starts at +0 and takes, in
 *              this order,  first order:   the pair (p - 1, p): +k,  (p, p + 1): -k,  (p - W, p): +k,  (p, p + W): -k
 *                           second order:  the triple centred at p - 1: +k,  at p: -2 k,  at p + 1: +k,  then the same three of
 *                                          the column (p - W, p, p + W)
 *              with k = (w e) sg(r) of that term; then grad_D(p) = acc * s, times -(x(p) x(p)) with GS_GEOM_INVERSE, rounded once.
 *              The selections and e are held fixed.  Every element of grad_D is written.
 *
 * ---- kernel shape ----
 * One 256-thread block per tile of GS_GEOM_TILE_H x GS_GEOM_TILE_W pixels, tiles numbered along x first.  The tile's depth with a
 * halo of GS_GEOM_HALO on every side, and every other plane the selection needs, are staged in LDS once; every neighbourhood is
 * then read from LDS.  A 16-byte aligned plane whose W is a multiple of 4 is moved four pixels per lane, any other pixel by
 * pixel, with equal bits.  Thread t works on the pixels (t % 64, t / 64 + 4 k), k = 0 .. 3, of its tile.  Sums are float64 in a
 * fixed order: each thread its pixels in ascending k (a pixel's horizontal term before its vertical one), a butterfly over the
 * wave (xor 32, 16, ..., 1), the four waves in order; then one finishing block of GS_GEOM_FINISH_THREADS threads, thread i
 * adding the per-tile sums i, i + threads, ..., and the same butterfly and wave order.
 * Launches: forward GS_GEOM_FORWARD_LAUNCHES (tile pass, finish), backward 1, gs_depth_normals 1.
 * Work memory (per-tile sums) belongs to the context and is counted by gs_ctx_device_bytes.
 *
 * GS_ERR_INVALID_ARGUMENT, before anything needs a device: ctx NULL; D, N, w_n, terms, normals or grad_D NULL (I, w_p and
 * upstream alone may be); H or W below 1, or more than GS_APPEARANCE_MAX_PIXELS pixels; flag bits outside
 * GS_GEOM_NORMAL_FLAGS_ALL / GS_GEOM_SMOOTH_FLAGS_ALL; fx or fy not finite or not > 0; cx or cy not finite; edge_lambda or
 * max_rel_jump not finite or negative.  An image too small to hold one term (2x2 for normals) is GS_OK with zero terms and a
 * zero gradient.
 */
#ifndef GS_GEOMETRY_H
#define GS_GEOMETRY_H
#include "gs_rasterizer.h"
#include "gs_appearance.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of the normal loss */
#define GS_GEOM_PRIOR_UNIT_RANGE 1
#define GS_GEOM_PRIOR_FLIP_YZ 2
#define GS_GEOM_NORMAL_FLAGS_ALL 3
/* flags of the smoothness */
#define GS_GEOM_INVERSE 4
#define GS_GEOM_SECOND_ORDER 8
#define GS_GEOM_SMOOTH_FLAGS_ALL 12

#define GS_GEOM_TILE_W 64
#define GS_GEOM_TILE_H 16
#define GS_GEOM_HALO 2
#define GS_GEOM_FINISH_THREADS 256          /* threads of the finishing block: it loops past this many per-tile sums */
#define GS_GEOM_LOSS_TERMS 8
#define GS_GEOM_FORWARD_LAUNCHES 2
#define GS_GEOM_BACKWARD_LAUNCHES 1

int gs_depth_normals(gs_ctx* ctx, const float* D, int32_t H, int32_t W, float fx, float fy, float cx, float cy, float max_rel_jump,
                     float* normals, gs_stream stream);

int gs_normal_loss_forward(gs_ctx* ctx, const float* D, const float* N, const float* w_n, const float* w_p, int32_t H, int32_t W,
                           float fx, float fy, float cx, float cy, float max_rel_jump, int32_t flags, float* terms, gs_stream stream);

int gs_normal_loss_backward(gs_ctx* ctx, const float* D, const float* N, const float* w_n, const float* w_p, int32_t H, int32_t W,
                            float fx, float fy, float cx, float cy, float max_rel_jump, int32_t flags, const float* terms,
                            const float* upstream, float* grad_D, gs_stream stream);

int gs_depth_smooth_forward(gs_ctx* ctx, const float* D, const float* I, const float* w_p, int32_t H, int32_t W, float edge_lambda,
                            int32_t flags, float* terms, gs_stream stream);

int gs_depth_smooth_backward(gs_ctx* ctx, const float* D, const float* I, const float* w_p, int32_t H, int32_t W, float edge_lambda,
                             int32_t flags, const float* terms, const float* upstream, float* grad_D, gs_stream stream);

#ifdef __cplusplus
}
#endif
#endif
