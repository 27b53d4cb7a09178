/* gs_view_hints.h -- a look into a context's view table, for tests and diagnostics.
 *
 * A context keeps, per view, the tile order (heaviest first) its last backward of that view computed, and dispatches the next
 * forward blend of the view in that order (csrc/gs_common.h: "the view table").  The table lives on the
 * device and is keyed there by the pose of object 0; it only moves work in time: any order gives the same bits.  GS_VIEW_HINTS
 * sets the number of slots (at most 1024, 1 = one slot that every pose matches, 0 = no table; unset = 64 for images of 4096 tiles
 * or more, where the order of dispatch matters, and 1 below).
 *
 * Same library, same rules as gs_rasterizer.h: status codes, gs_last_error().  Not part of GS_ABI_VERSION's function list.
 */
#ifndef GS_VIEW_HINTS_H
#define GS_VIEW_HINTS_H
#include "gs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_VIEW_KEY_FLOATS 7     /* q_pointcloud_camera (xyzw) and t_pointcloud_camera (xyz) of object 0, as the caller gave them */

/* Waits for the device, then copies out of the context's table (all outputs are HOST memory, each may be NULL):
 *   n_slots, n_tiles   the table's slot count S and tile count T; both 0 when the context has no table (yet);
 *   keys, filled       (S, GS_VIEW_KEY_FLOATS) floats and (S) flags (1: the slot holds a complete order), as far as slot_cap slots;
 *   order              the T tiles of slot `slot`, as far as order_cap of them; slot S is the order of the frames that have no
 *                      pose to be keyed by (gs_forward_projected); ignored when slot < 0;
 *   frame_slots        with `frame`: { read slot, write slot } of that frame, { -2, -2 } for a frame that looked no pose up
 *                      (any frame of a one-slot table, a frame built from records, a frame of an empty scene, a frame of an
 *                      earlier layout of the table).
 *                      read slot -1: no slot was filled when the frame's forward ran.
 * GS_ERR_INVALID_ARGUMENT: ctx NULL, slot > S, negative capacities; GS_ERR_STATE: `frame` is not a live frame of ctx. */
int gs_view_hints_read(gs_ctx* ctx, const gs_frame* frame, int32_t slot, int32_t* n_slots, int32_t* n_tiles,
                       float* keys, int32_t* filled, int32_t slot_cap, int32_t* order, int32_t order_cap, int32_t* frame_slots);

#ifdef __cplusplus
}
#endif
#endif
