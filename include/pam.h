/*
 * pam.h -- C ABI of libpam_hip.so: the MI355X (gfx950) implementation of the per-frame multi-view 3D pose
 * hot path of B10532021/Part-Aware_Measurement_for_3D_Pose_Estimation_and_Tracking.
 *
 * The reference has no FFI (pure Python); the seams this ABI replaces are the Python call sites below
 * (paths relative to /root/reference/src).  Host code (the package's ivclabpose.py / tracker.py) binds these with
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: extern "C"; plain pointers and sizes; every function returns 0 on success or a negative PAM_E_*
 * code, with text available from pam_last_error(); no exceptions or callbacks cross the ABI; a handle owns its
 * device memory, is bound to one GPU and is not thread-safe.  "host" pointers are ordinary host memory, "dev"
 * pointers are device memory (e.g. torch tensor .data_ptr()); `stream` is a hipStream_t passed as void* (NULL =
 * the legacy null stream, which is what torch's default stream is).  Keypoints are rows (y, x, score) in float64 -- the tracker-internal layout the
 * reference builds at ivclabpose.py:236-244.
 */
#ifndef PAM_H
#define PAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAM_J 17            /* joints; hard-coded 17 in the reference too (ivclabpose.py:96) */
#define PAM_MAX_VIEWS 32    /* per-joint view sets are 32-bit masks */
#define PAM_MAX_TAPS 16
#define PAM_EXP_TABLE 64
#define PAM_YOLO_MAX_CAND 1024 /* boxes above the score threshold kept per image before NMS */

#define PAM_OK 0
#define PAM_E_ARG (-1)      /* bad argument / capacity */
#define PAM_E_HIP (-2)      /* HIP runtime error */
#define PAM_E_STATE (-3)    /* call order (e.g. cameras not set) */
#define PAM_E_OVERFLOW (-4) /* a scene ran out of track / hypothesis slots (see out status word) */

/* Matcher hyper-parameters: ivclabpose.py:140-156 (iter_args) + derived tables computed by the host exactly as
 * the reference's Python does (math.exp / scipy _gaussian_kernel1d), so the device uses bit-identical constants. */
typedef struct PamParams {
    double conf_threshold;       /* PIPELINE_COMBINATION.CONF_THRESHOLD            */
    double epi_threshold;        /* EPI_THRESHOLD   (hypothesis cost scale)         */
    double init_threshold;       /* INIT_THRESHOLD  (init-path joint filter, f32)   */
    double joint_threshold;      /* JOINT_THRESHOLD (update-path joint filter)      */
    double alpha2d;              /* ALPHA2D                                         */
    double lambda_a;             /* LAMBDA_A                                        */
    double lambda_t;             /* LAMBDA_T                                        */
    int32_t n_init;              /* N_INIT                                          */
    int32_t max_age;             /* MAX_AGE                                         */
    int32_t count_gate;          /* 10: the literal at IterativeTracker.py:145      */
    int32_t n_taps_body;         /* radius+1 taps of gaussian_filter1d(sigma)       */
    int32_t n_taps_arm;          /* radius+1 taps of gaussian_filter1d(arm_sigma)   */
    int32_t reserved;
    double taps_body[PAM_MAX_TAPS];   /* w[0]=centre ... w[r]                       */
    double taps_arm[PAM_MAX_TAPS];
    double exp_lambda_a[PAM_EXP_TABLE]; /* exp(lambda_a * dt), dt = 0..63           */
    double w_lambda_t[4];               /* exp(-lambda_t * T), T = 0..3             */
} PamParams;

typedef struct PamHandle PamHandle;

/* Layout of the per-scene output record (int32 words then float64 words); filled by pam_out_layout(). */
typedef struct PamOutLayout {
    int32_t n_views, max_dets, max_tracks, n_scenes;
    int32_t int_words;      /* int32 words per scene  */
    int32_t dbl_words;      /* float64 words per scene */
    /* int32 section: header then per-track blocks (list order = the reference's self.tracks order) */
    int32_t hdr_words;      /* [0]=n_tracks [1]=status word: bits 0-15 = status bits OF THIS FRAME: 1 = out of track slots, 2 = out of
                             * hypothesis slots, 4 = an assignment problem was infeasible, 8 = a device-side detection count outside
                             * [0, max_dets] was clamped (pam_frame_dev), 16 = the frame's input was VOID (pam_set_input_guard): the frame was
                             * not applied -- state untouched, no tracks in the record, [3] = first frame of this run of void frames (never
                             * sticky); bits 16-31 = bits 1-8 OR-ed over EVERY frame since
                             * pam_create / pam_reset (sticky: a host that decodes only the last record of a run still sees them)
                             * [2]=frame_id [3]=n_hyp (debug) */
    int32_t trk_words;      /* words per track block */
    /* track block: 0 id,1 state,2 hits,3 age,4 time_since_update,5 emitted,6 n_2d_views,7 V (views offered to the
     * newest pose),8 history length,9 newest pose time, then order[n_views], matched_det[n_views] (index of the
     * detection matched THIS frame per camera id or -1), time2d[n_views] (per camera id), nviews[17] */
    int32_t off_order, off_matched, off_time2d, off_nviews;
    /* float64 section: [0..15] in-kernel clocks (s): [0] start, [1] after association, [2] after update, [3] after init,
     * [4..11] finer phase stamps (view selection, conflicts, DLT, success, smoothing, append, end of init, end of record);
     * then per track pose3d[17*3], velocity[17*3] */
    int32_t dbl_hdr_words;
    int32_t dbl_trk_words;
} PamOutLayout;

/* ---- life cycle --------------------------------------------------------------------------------------------
 * replaces: ivclabpose.__init__ (ivclabpose.py:136-158) + IterativeTracker.__init__ (IterativeTracker.py:36-45).
 * n_scenes > 1 runs that many independent tracker instances per launch (batched scenes, same rig). */
int pam_create(PamHandle** out, int device, int n_views, int max_dets, int max_tracks, int max_hyps,
               int n_scenes, const PamParams* params);
int pam_destroy(PamHandle* h);
const char* pam_last_error(const PamHandle* h);   /* h may be NULL: last create error */
const char* pam_version(void);

/* replaces: ivclabpose.GetCameraParameters / Camera.__init__ results (ivclabpose.py:35-46,162-181).  The host computes
 * P, F, RK_INV (float32) and position (float64) exactly as the reference does and hands them over. */
int pam_set_cameras(PamHandle* h, const float* P /*C*3*4*/, const float* F /*C*C*3*3*/,
                    const float* RK_INV /*C*3*3*/, const double* position /*C*3*/);

/* replaces: IterativeTracker.track_restart (IterativeTracker.py:47-50) */
int pam_reset(PamHandle* h);

int pam_out_layout(const PamHandle* h, PamOutLayout* out);

/* How the per-frame step runs on this handle (read-only, fixed by pam_create's arguments): block = threads per workgroup (256, or
 * 1024 on rigs of more than 8 views), launches = kernel launches per frame (3 for a single-scene rig of more than 8 views: association,
 * the conflict sets over the whole chip, the rest; else 1, one workgroup per scene), hot_in_lds = 1 when a scene's hot scratch and
 * integer state fit in 128 KB and are held in LDS for the frame, 0 when the kernel works on them in global memory. */
int pam_frame_plan(const PamHandle* h, int32_t* block, int32_t* launches, int32_t* hot_in_lds);

/* ---- the per-frame step ------------------------------------------------------------------------------------
 * replaces: IterativeTracker.tracking (IterativeTracker.py:115-180) + output collection (ivclabpose.py:259-287):
 * association, per-track part-aware view filter + weighted DLT + smoothing + motion, greedy hypothesis
 * initialisation, life cycle.  State stays on the device.
 *   n_det : n_scenes*C int32         detections per view
 *   det   : n_scenes*C*max_dets*17*3 float64 rows (y, x, score)
 * pam_frame: host buffers in, host record out (out_i: n_scenes*int_words, out_d: n_scenes*dbl_words); synchronous.
 * pam_frame_dev: device buffers in, record left in the handle's device output buffer; asynchronous on `stream`.
 * pam_fetch: async copy of the device output record to (pinned) host memory on `stream`. */
int pam_frame(PamHandle* h, int frame_id, const int32_t* n_det, const double* det, int32_t* out_i, double* out_d);
int pam_frame_dev(PamHandle* h, void* stream, int frame_id, const int32_t* dev_n_det, const double* dev_det);
/* the same step on VIEW-SHARDED input, read in place (no unpack kernel, no copies): dev_records = the buffer the all-gather of the
 * ranks' send buffers filled (pam_allgather_keypoints' dev_recv; record layout there), dev_view_row[v] (n_views int32) = which of its
 * records holds view v.  One scene per handle. */
int pam_frame_dev_views(PamHandle* h, void* stream, int frame_id, const double* dev_records, const int32_t* dev_view_row);
int pam_fetch(PamHandle* h, void* stream, int32_t* host_out_i, double* host_out_d);
int pam_sync(PamHandle* h, void* stream);
/* Input guard of the frame step (round 6).  The reference's PersonPoseDetect returns host lists before PersonTrack_Project3DPose runs
 * (/root/reference/src/ivclabpose.py:208-287): a frame can never be tracked on keypoints their producer disowns.  Here the tracker consumes
 * the decode on the device, so the producer's verdict has to be readable there: while *dev_word != 0 (a device int32 the producer raises:
 * pam_flag_gate's dev_void; for view-sharded input also the second double of any record's count row) pam_frame* does NOT apply the frame --
 * the state stays as it is and the record carries status bit 16.  The host re-submits from record word [3] once it has cleared the word.
 * dev_word = NULL removes the guard. */
int pam_set_input_guard(PamHandle* h, const int32_t* dev_word);

/* ---- person boxes without the detector, and box lists as crop tables (no reference counterpart: the reference runs its detector on
 * every frame, /root/reference/src/testmodel.py:59-63) ---------------------------------------------------------------------------
 * pam_track_boxes: person boxes of frame_id from the tracker state as the frame launches already on `stream` leave it (the state lives in
 * global memory between frames; the kernel only reads it and does not look at the input guard).  Tracks in list order (the record's
 * order), Tentative and Confirmed alike.  A track is eligible iff 0 <= gap <= max_gap with gap = frame_id - (time of its newest pose);
 * its pose is moved to frame_id by the frame step's own constant-velocity expression (newest + (double)(velocity * (float)gap), a
 * float32 product added in double) and projected into every view; a (track, view) pair gets a box iff all 17 joints lie in front of
 * the camera.  Box, in double: centre = middle of the joints' min / max, half sizes = 0.5 * grow * (max - min) + pad_px, clamped to
 * [0, frame_w] x [0, frame_h], dropped if the clamped width or height is < min_size_px, rounded once to float32; score 1.0f.
 * Output in pam_yolo_detect's layout for C = n_views images: dev_boxes C * max_det rows (x1, y1, x2, y2, score) (unused rows zero),
 * dev_count[v] = rows written for view v (at most max_det), dev_count[C + v] = boxes before that clamp, dev_ids (C * max_det, or NULL)
 * the rows' track ids (-1 where unused), dev_info[0] = 1 if any view was clamped, dev_info[1] = eligible tracks.
 * PAM_E_ARG, before any device call: NULL handle, max_det < 1, a NULL output (dev_ids excepted), a scene the handle does not have.
 *
 * pam_crop_table (csrc/pam_boxes.hip; no handle): detector-layout box lists -> the tables pam_preprocess_crops* / pam_head_decode* take,
 * for a host that does not know the counts.  Local view i < n_views reads the list of image g = dev_views ? dev_views[i] : i (rows at
 * dev_boxes + g * max_det_in * 5, count dev_count[g], clamped to [0, max_det_in]) and keeps its first min(count, max_dets) rows; rows are
 * ordered by (view, slot) and only the first `cap` of them stay (dev_n_det[i] = rows view i kept).  Row r: dev_view_of[r] = i,
 * dev_slot_of[r] = slot, dev_xywh[r] = (max(0, x1), max(0, y1), min(x2, frame_w) - x, min(y2, frame_h) - y) -- clamped and subtracted in
 * double, one rounding to float32, nothing dropped: bit-identical to the boxes ivclabpose.PersonDetect hands HRNetPose.predict.  Rows
 * [total, cap) repeat row total - 1 (same view, slot and box: they decode the same crop into the same slot), or (view 0, slot 0, the
 * whole frame) when total = 0, so crop, forward and decode can be launched for cap rows.  dev_info[0] = total, [1] = rows wanted before
 * the cap cut, [2] = 1 if a view's list was cut to max_dets | 2 if the rows were cut to cap, [3] = 0.  One workgroup; n_views <= 256.
 * PAM_E_ARG: a NULL pointer (dev_views excepted), n_views / max_det_in / max_dets / cap < 1. */
int pam_track_boxes(PamHandle* h, void* stream, int scene, int frame_id, int frame_w, int frame_h, float grow, float pad_px,
                    float min_size_px, int max_gap, int max_det, float* dev_boxes, int32_t* dev_count, int32_t* dev_ids,
                    int32_t* dev_info);
int pam_crop_table(void* stream, int n_views, const int32_t* dev_views, const float* dev_boxes, const int32_t* dev_count,
                   int max_det_in, int frame_w, int frame_h, int max_dets, int cap, int32_t* dev_view_of, int32_t* dev_slot_of,
                   float* dev_xywh, int32_t* dev_n_det, int32_t* dev_info);

/* ---- duplicate 2D poses out of each view (csrc/pam_pose_nms.hip; no handle, asynchronous on `stream`; no reference counterpart: the
 * rescoring + greedy OKS-NMS of the HRNet / Simple Baselines test protocol, TEST.OKS_THRE / TEST.IN_VIS_THRE) ------------------------
 * pam_pose_nms filters the decode's buffer in place, one workgroup per view, all in float64.  View v < n_views holds
 * n = clamp(dev_n_det_in[v], 0, max_dets) rows (y, x, s)[17] at dev_det + v * det_slots * 51 (det_slots >= max_dets: max_dets for
 * HRNetPose.predict's buffer, max_dets + 1 for ViewGather's view records).  The crop rows that produced the buffer (n_rows of
 * dev_view_of / dev_slot_of / dev_xywh, the tables pam_preprocess_crops* took; rows that repeat a (view, slot) carry the same box) give
 * each row its area = (double)w * (double)h (0 for a slot no crop row names).  Box score b of (v, slot) = dev_score[g * view_stride +
 * slot * slot_stride] with g = dev_views ? dev_views[v] : v (strides in floats: a detector-layout list (G, max_det, 5) is read in place
 * as dev_boxes + 4 with strides (5 * max_det, 5)); dev_score = NULL means 1.0.
 *   score   = (double)b * mean{ s_j : s_j > in_vis_thre }   (summed over j = 0..16 in order; 0.0 when no joint passes)
 *   oks(p,q) = (1/17) sum_j exp(-e_j),  e_j = ((dx_j)^2 + (dy_j)^2) / vars[j] / ((area_p + area_q) / 2 + 2.220446049250313e-16) / 2
 *             (all 17 joints always count; vars: 17 host doubles, (2 sigma_j)^2, copied into the launch)
 *   order   = descending score, equal scores by lower slot (a NaN score goes last)
 *   greedy  = the first row of the order that is alive is kept and kills every alive row q with oks(kept, q) > oks_thre (a NaN OKS
 *             kills nothing; NOT transitive: what a killed row would have killed stays unless a kept row kills it); repeat.
 * Output: the kept rows in their original slot order, compacted to slots 0 .. kept - 1 (a view without duplicates is left bit-identical),
 * rows [kept, n) set to 0.0, rows >= n untouched; dev_n_det_out[v] = kept; dev_keep_from[v * max_dets + slot] = the original slot of the
 * row now at `slot` (-1 from kept on); dev_pose_score[v * max_dets + slot] = its score (0.0 from kept on).  dev_n_det_out must not be
 * dev_n_det_in: a forward that is issued again decodes and filters again from the original counts.
 * Counts and crop rows are clamped or skipped (no row index leaves its view).  The score grid is the caller's to guarantee, as the box list
 * of pam_crop_table is: dev_views[v] and every (g, slot < max_dets) address must lie inside dev_score -- the kernel cannot know its extent.
 * The library is built with -ffp-contract=off, so e_j is computed as written (no fused multiply-add); exp is the device library's and may
 * differ from another implementation's in the last bits.
 * PAM_E_ARG, before any device call: a NULL pointer (dev_score and dev_views excepted), n_views < 1, max_dets outside 1..32,
 * det_slots < max_dets, n_rows < 0, dev_n_det_out == dev_n_det_in. */
int pam_pose_nms(void* stream, int n_views, int max_dets, int det_slots, double* dev_det, const int32_t* dev_n_det_in, int n_rows,
                 const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_xywh, const float* dev_score,
                 long long view_stride, long long slot_stride, const int32_t* dev_views, const double* vars, double oks_thre,
                 double in_vis_thre, int32_t* dev_n_det_out, int32_t* dev_keep_from, double* dev_pose_score);

/* ---- lens distortion out of the decoded keypoints (csrc/pam_lens.hip, csrc/pam_lens.hpp; no reference counterpart: the reference's
 * Camera.undistort / undistort_points are identity stubs and its matching path takes every camera for an ideal pin-hole) -----------------
 * The model is Brown-Conrady in the OpenCV / Panoptic order (k1, k2, p1, p2, k3) on normalised coordinates, K upper-triangular.  A camera
 * is a row of 10 doubles: fx, fy, cx, cy, skew, k1, k2, p1, p2, k3.  All float64.  With u the column and w the row of a pixel:
 *   normalise   y = (w - cy) / fy;  x = (u - cx - skew * y) / fx            pixels   u = fx * x + skew * y + cx;  w = fy * y + cy
 *   forward     r2 = x * x + y * y;  rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
 *               xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
 *               yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
 *   inverse     of (dx, dy): (x, y) = (dx, dy), then 8 times, always 8 (no data-dependent exit):
 *               r2, rad as above;  drad = k1 + r2 * (2.0 * k2 + 3.0 * r2 * k3)
 *               ex = xd(x, y) - dx;  ey = yd(x, y) - dy
 *               a = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
 *               b = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
 *               d = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
 *               det = a * d - b * b;  x = x - (d * ex - b * ey) / det;  y = y - (a * ey - b * ex) / det
 *               The point CANNOT BE INVERTED when det > 0.0 is false at any of the 8 iterates (a point beyond the fold of the model, or
 *               NaN), or when |xd(x, y) - dx| <= 1e-9 or |yd(x, y) - dy| <= 1e-9 is false at the end (normalised units).
 * The library is built with -ffp-contract=off, so these are computed as written (no fused multiply-add); the division is the device's.
 *
 * pam_undistort_keypoints works in place on the decode's buffer, in pam_pose_nms' layout: view v < n_views holds
 * n = clamp(dev_n_det[v], 0, max_dets) rows (y, x, s)[17] at dev_det + v * det_slots * 51 (det_slots = max_dets, or max_dets + 1 for
 * ViewGather's view records).  One lane per keypoint, n_views * max_dets * 17 of them.  The camera of view v is row
 * g = dev_views ? dev_views[v] : v of dev_lens (the caller guarantees that the row exists, as with pam_pose_nms' score grid).  Each (y, x)
 * of a row below its view's count is normalised (u = x, w = y), inverted and taken back to pixels.  Never touched: the score column; rows
 * at or beyond the view's count; every row of a camera whose five coefficients are all exactly 0.0 (a rig without distortion stays
 * bit-identical).  A point that is not finite or cannot be inverted keeps its input coordinates and adds 1 to dev_info[0] (an ordinary
 * global atomic add; the entry point zeroes dev_info[0..1] on `stream` in front of the launch).  dev_info[1] = the sum of 17 * n over the
 * views: the points below the counts, pin-hole cameras' and kept ones included.
 * PAM_E_ARG, before any device call: a NULL pointer (dev_views excepted), n_views < 1, max_dets outside 1..32, det_slots < max_dets.
 *
 * pam_set_lens stores a host table of C rows (C = the handle's views) in the handle, on the device, for pam_track_boxes: while a table is
 * set, each joint's projection (u, w) is normalised with its camera's K, pushed through the forward model and taken back to pixels before
 * the min / max, so the box lies round the person in the RAW image (a camera of the table whose coefficients are all 0.0 is skipped).
 * NULL, or a table whose coefficients are all 0.0, removes the table: pam_track_boxes then runs the expressions and gives the bits it
 * gave before.  The frame step never reads the table: its keypoints are undistorted before they reach it.  Synchronises the device,
 * except when there is no table to set and none to remove (then no device call is made).
 * PAM_E_ARG: NULL handle, a value that is not finite, a zero fx or fy in a table that has a non-zero coefficient. */
int pam_undistort_keypoints(void* stream, int n_views, int max_dets, int det_slots, double* dev_det, const int32_t* dev_n_det,
                            const int32_t* dev_views, const double* dev_lens, int32_t* dev_info);
int pam_set_lens(PamHandle* h, const double* lens /* host, C * 10, or NULL */);

/* ---- One-Euro filter on the tracks' 3D output (csrc/pam_one_euro.hip, csrc/pam_one_euro.hpp) ------------------------------------------
 * replaces: OneEuroFilter.__call__ (/root/reference/src/tracking/OneEuroFilter.py:41-77) as IterTrack.__init__ sets it up per joint and
 * axis (IterativeTracker.py:225-237: freq 25, mincutoff 0.8, beta 0.4, dcutoff 0.4); the reference's three calls in smooth_3dpose are
 * commented out (:373-376), so this is an OUTPUT filter: it reads the tracker state and never writes it; the frame step, its record and
 * every decision stay what they are.  All float64.  One scalar channel with state (n, freq, t_last, x_prev, x_hat, dx_hat) takes sample x
 * at time t (the class's own expressions, its truthiness test on the time stamps included: a time stamp of 0.0 never updates freq):
 *   if n > 0 and t_last != 0.0 and t != 0.0:  freq = 1.0 / (t - t_last)
 *   t_last = t
 *   alpha(c) = 1.0 / (1.0 + (1.0 / (2 * pi * c)) / (1.0 / freq))              pi = 3.141592653589793
 *   dx   = 0.0 if n == 0 else (x - x_prev) * freq
 *   edx  = dx  if n == 0 else alpha(dcutoff) * dx + (1.0 - alpha(dcutoff)) * dx_hat
 *   cut  = mincutoff + beta * fabs(edx)
 *   x_hat = x  if n == 0 else alpha(cut) * x + (1.0 - alpha(cut)) * x_hat
 *   dx_hat = edx;  x_prev = x;  n += 1;  the output is x_hat
 * The library is built with -ffp-contract=off, so these are computed as written; the division is the device's.
 * The 51 channels of a track (17 joints x 3 axes) share n, freq and t_last; t = (double)frame_id / cfg.freq, so cfg.freq is the frame rate
 * and the filter's initial frequency.
 *
 * pam_set_one_euro stores the configuration and allocates the zeroed filter state in the handle (per scene and track slot: id, last_frame,
 * n, freq, t_last, x_prev[51], x_hat[51], dx_hat[51]); setting it again restarts every filter, and so does pam_reset while one is set.
 * NULL switches the filter off and frees the state.  Synchronises the device.  PAM_E_ARG: NULL handle, a value that is not finite, freq,
 * mincutoff or dcutoff <= 0 (beta may be 0).
 *
 * pam_one_euro (k_one_euro: one workgroup per scene, asynchronous on `stream`) filters the newest pose of every listed track, Tentative
 * and Confirmed alike, as the frame launches already on `stream` leave the state; it does not look at the input guard.  For the track at
 * list position i (the record's order) in slot s, with `fresh` = the time of its newest pose equals frame_id:
 *   - a slot that holds no samples, or whose stored id is not the track's, starts over: n = 0, freq = cfg.freq (a slot reused by a track
 *     born in the frame its predecessor died);
 *   - fresh, same id and last_frame == frame_id: the sample has been consumed, the state is left alone -- a second call, or a call after a
 *     frame that was skipped and re-submitted, changes nothing and writes the same buffers;
 *   - fresh with frame_id < last_frame (time went back without a pam_reset): starts over, then consumes the sample;
 *   - fresh otherwise: consumes the sample (one step of every channel) and sets last_frame = frame_id;
 *   - not fresh: the row is the held x_hat; a track without state (the filter was switched on mid-run) gives its newest pose as it is,
 *     with samples = 0.
 * dev_pose: n_scenes * max_tracks * 51 doubles, row i = the 17 x 3 filtered joints of list position i, rows from n_tracks on 0.0; on a
 * track's first sample the row holds the raw pose's bits.  dev_meta: n_scenes * (2 + 3 * max_tracks) int32, [0] = n_tracks, [1] = fresh
 * rows (the samples of this frame that are in dev_pose), then per row (id, fresh, samples = n after the call); rows from n_tracks on are
 * (-1, 0, 0).  PAM_E_STATE without a configuration; PAM_E_ARG, before any device call: a NULL handle or buffer. */
typedef struct PamOneEuro { double freq, mincutoff, beta, dcutoff; } PamOneEuro;
int pam_set_one_euro(PamHandle* h, const PamOneEuro* cfg /* host, or NULL = off */);
int pam_one_euro(PamHandle* h, void* stream, int frame_id, double* dev_pose, int32_t* dev_meta);

/* ---- per-operator entry points (parity tests; host buffers, synchronous) -----------------------------------*/
/* Camera.projectPoints_parallel, ivclabpose.py:91-98: n poses (17x3) -> (17x2) in (y, x) */
int pam_op_project(PamHandle* h, int cid, int n, const double* poses3d, double* out_yx);
/* affinity build, IterativeTracker.py:137-149: tracks_pose n*17*3, dt n, dets m*17*3 -> aff n*m */
int pam_op_track_affinity(PamHandle* h, int cid, int n, int m, const double* tracks_pose, const int32_t* dt,
                          const double* dets, double* aff);
/* scipy.optimize.linear_sum_assignment call sites IterativeTracker.py:79,150: cost nr*nc (minimise) ->
 * rows/cols (min(nr,nc) pairs, sorted by row) */
int pam_op_lsap(PamHandle* h, int nr, int nc, const double* cost, int32_t* rows, int32_t* cols, int32_t* n_pairs);
/* epipolar_affinity_parallel, matching.py:115-151: V views of one person -> V*V*17 symmetric distances */
int pam_op_epi_dist(PamHandle* h, int V, const int32_t* cids, const double* pose_mat, double* dist);
/* epipolar_distance, matching.py:50-91 (OpenCV epilines form): -> 17*2 */
int pam_op_epi_pair(PamHandle* h, int c1, const double* person1, int c2, const double* person2, double* out);
/* epipolar_affinity, matching.py:93-113 (float32 storage): -> V*V*17 float32 */
int pam_op_epi_dist_init(PamHandle* h, int V, const int32_t* cids, const double* pose_mat, float* dist);
/* Greedy_matching, matching.py:243-295.  mode 0 = 'update' (aff float64, needs pose_j V*3 and next_pose_j 3),
 * mode 1 = 'init' (aff given as float32).  aff is V*V for ONE joint.  -> keep bitmask over views */
int pam_op_greedy(PamHandle* h, int mode, int V, const int32_t* cids, const void* aff, const double* pose_j,
                  const double* next_pose_j, uint32_t* keep_mask);
/* SVD_pose_kernel_jf, construction.py:89-114: keep_mask[17] view sets, Ts[V] ages -> 17*3 */
int pam_op_dlt(PamHandle* h, int V, const int32_t* cids, const int32_t* Ts, const double* pose_mat,
               const uint32_t* keep_mask, const double* next_pose, double* out);
/* pam_op_dlt with the solver's paths selectable and reported.  nsplit 1: every joint's rows folded by one lane, as pam_op_dlt does;
 * nsplit 4: the form the frame step takes on tracks of more than 8 views -- lane q folds the kept views q, q + 4, ... into a triangular
 * factor of its own, the four factors are packed to device memory, merged in the order 0..3 and solved.  solver 0: inverse iteration, then
 * one-sided Jacobi if it did not converge (what the frame step runs); solver 1: Jacobi alone.  path[17]: 0 = fewer than two kept views,
 * next_pose copied; 1 = inverse iteration converged; 2 = Jacobi.  PAM_E_ARG: V outside 1..32, nsplit not 1 or 4, solver not 0 or 1, a
 * NULL argument, a camera id outside the handle's views. */
int pam_op_dlt_paths(PamHandle* h, int V, const int32_t* cids, const int32_t* Ts, const double* pose_mat,
                     const uint32_t* keep_mask, const double* next_pose, int nsplit, int solver, double* out, int32_t* path);
/* IterTrack.smooth_3dpose, IterativeTracker.py:371-383: hist L*17*3 + raw 17*3 -> 17*3 */
int pam_op_smooth(PamHandle* h, int L, const double* hist, const double* raw, double* out);
/* IterTrack.update_motion, IterativeTracker.py:385-395: hist L*17*3 (L>=2) -> float32 17*3 */
int pam_op_velocity(PamHandle* h, int L, const double* hist, float* vel);
/* Hypothesis.calculate_cost, hypothesis.py:53-68 */
int pam_op_hyp_cost(PamHandle* h, int n_members, const int32_t* cids, const double* poses, int o_cid,
                    const double* o_pose, double* cost, int32_t* veto);
/* OneEuroFilter.__call__, OneEuroFilter.py:63-77, through the device function k_one_euro runs: K independent channels (one lane each)
 * walk the n samples x[i * K + k] at times t[i], every filter new (n = 0, freq = cfg->freq) -> out n*K.  n >= 0, 1 <= K <= 4096, the
 * configuration as pam_set_one_euro takes it (the handle's own is neither read nor changed). */
int pam_op_one_euro(PamHandle* h, int n, int K, const double* t, const double* x, const PamOneEuro* cfg, double* out);

/* ---- image side of a1 (HRNetPose.predict pre/post-processing; call site ivclabpose.py:210) ------------------
 * pam_preprocess_crops: n person boxes (x, y, w, h float32, in pixels of frame view_of[i]) cropped from BGR uint8
 * frames (dev pointers, H x W x 3, row pitch W*3), bilinear-resized to out_h x out_w, BGR->RGB, /255, ImageNet
 * mean/std, written as bf16 NHWC (n, out_h, out_w, 3) -- the channels-last input of the conv stack.
 * pam_decode_heatmaps: heat-maps (n, hm_h, hm_w, 17) float32 NHWC or (n,17,hm_h,hm_w) NCHW (nchw flag) -> per person
 * hard arg-max per joint mapped through the box; writes float64 rows (y, x, score) into the tracker's det buffer
 * slot (view_of[i], slot_of[i]).  All pointers are device pointers; asynchronous on `stream`. */
/* final 1x1 convolution of the pose network (`final_layer` of the HRNet module inside HRNetPose.predict): features NHWC bf16
 * (n_pix pixels x C channels, C % 8 == 0) -> heat-maps NHWC float32 (n_pix x J, J = 17); w [J][C] float32, bias [J] or NULL;
 * float32 FMA chain over the channels in order, starting from the bias. */
int pam_head_heatmaps(void* stream, int n_pix, const void* feat_bf16, int C, const float* w, const float* bias, int J,
                      float* out);
/* head + decode in one pass (what the product path runs): the same 1x1 convolution (bit-identical values) with the per-joint
 * (max, first index) reduced on the fly -- the heat-maps are written only if dev_heatmaps_or_null is given.  feat: (n, hm_h, hm_w, C)
 * bf16 NHWC; det / kp / view_of / slot_of / boxes as pam_decode_heatmaps; dev_scratch: pam_head_decode_scratch_bytes(n, hm_h, hm_w)
 * bytes of device memory owned by the caller (per-tile candidates).  Ties go to the lowest flat index; a map with no value above -inf
 * (all -inf or NaN) decodes as cell 0 with score -inf, here and in pam_decode_heatmaps. */
long long pam_head_decode_scratch_bytes(int n, int hm_h, int hm_w);
int pam_head_decode(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias, int J,
                    float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes,
                    int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch);
/* the same pass with a SOFT arg-max decode (optional mode; the hard arg-max above is the parity mode): per joint the keypoint is the
 * softmax(beta * heat-map)-weighted mean (column, row) over the crop's heat-map -- sub-pixel -- mapped through the box like the hard
 * one; the confidence stays the heat-map maximum.  Per-tile partials (max, sum exp, weighted sums) merged streaming-softmax style;
 * dev_scratch: pam_head_decode_soft_scratch_bytes(n, hm_h, hm_w) bytes.  beta > 0. */
long long pam_head_decode_soft_scratch_bytes(int n, int hm_h, int hm_w);
int pam_head_decode_soft(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias, int J,
                         float beta, float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of,
                         const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch);
int pam_preprocess_crops(void* stream, int n, const void* const* dev_frames /*dev array of n_views frame ptrs*/,
                         int frame_h, int frame_w, const int32_t* dev_view_of, const float* dev_boxes,
                         int out_h, int out_w, int out_c /*3, or 8 = RGB + 5 zero channels*/, void* dev_out_bf16);
/* the same with (a) n_total >= n crops written: crops n .. n_total - 1 repeat crop n - 1 (a hipGraph replay captured for a bucket of
 * n_total crops takes a call of n without a padded box table), and (b) antialias != 0: the resize of upstream simple-HRNet (a PIL image
 * through torchvision's Resize, i.e. PIL's ImagingResample with the bilinear filter): taps = the frame pixels whose centres lie within
 * max(scale, 1) of the output pixel's centre inside the box rounded outwards, triangle weights, normalised, in float32 (PIL's uint8
 * rounding between its two passes is not reproduced).  Equal to the plain bilinear form wherever the box is not larger than the output.
 * At most 24 taps per axis (down-scaling by up to 11.5); a wider window keeps the 24 taps nearest the centre.  The outward-rounded box
 * is clamped to the frame and always keeps one column / row of it (a box wholly outside: the nearest one); an output pixel none of whose
 * taps has a positive weight is black (0 before the normalisation). */
int pam_preprocess_crops_ex(void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w,
                            const int32_t* dev_view_of, const float* dev_boxes, int out_h, int out_w, int out_c, void* dev_out_bf16,
                            int antialias);
/* ---- flip test (the official HRNet / Simple Baselines test protocol: TEST.FLIP_TEST, TEST.SHIFT_HEATMAP, TEST.POST_PROCESS) ----
 * pam_preprocess_crops_flip: the crops of one flip-test forward in one buffer of n_total >= 2 n rows: rows [0, n) as
 * pam_preprocess_crops_ex writes them (bit for bit), rows [n, 2n) the column reversal of row r - n (out[oy][ox] = plain[oy][out_w-1-ox]
 * bit for bit on both resize paths: the official input.flip(3), the same samples stored mirrored, not a resample of a mirrored box),
 * rows [2n, n_total) repeat row 2n - 1 (bucket padding, never decoded).  Other arguments as pam_preprocess_crops_ex. */
int pam_preprocess_crops_flip(void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w,
                              const int32_t* dev_view_of, const float* dev_boxes, int out_h, int out_w, int out_c, void* dev_out_bf16,
                              int antialias);
/* ---- the pose checkpoints' centre/scale box transform (official _box2cs + get_affine_transform + warpAffine + transform_preds) ----
 * The EFFECTIVE box of a person box (x, y, w, h) for a network input of out_w x out_h (csrc/pam_box_cs.hpp, one __host__ __device__
 * function), float64 from the float32 inputs in exactly this order, each of the four results rounded once to float32:
 *     cx = x + w * 0.5;  cy = y + h * 0.5
 *     if      (w * out_h > h * out_w)  h = w * out_h / out_w        too wide: grow the height
 *     else if (w * out_h < h * out_w)  w = h * out_w / out_h        too tall: grow the width
 *     We = w * box_scale;  He = We * out_h / out_w                  (box_scale: _box2cs's 1.25)
 *     xe = cx - We * 0.5;  ye = cy - He * 0.5
 * A box whose We is not > 0 (NaN included) gives (x, y, 0, 0) and an all-zero crop (before normalisation).  (The official code compares
 * w > aspect * h with a float aspect; the integer-ratio form differs from it on exact ties only.)  The decodes map a heat-map cell with
 * px / hm_w * box_w + box_x: handed the effective box as dev_boxes that IS transform_preds, and pam_pose_nms handed the same table takes
 * the official area prod(scale * 200) = We * He.
 * pam_preprocess_crops_affine: rows as pam_preprocess_crops_ex (flip = 0: n_total >= n, rows n .. repeat row n - 1) or as
 * pam_preprocess_crops_flip (flip != 0: n_total >= 2 n, rows [n, 2n) the column reversal of the plain rows bit for bit, rows from 2n on
 * repeat row 2n - 1), each row sampled from its box's effective box, which the launch also stores: dev_eff_xywh[r] for r < n (n x 4
 * float32; rows >= n are never written).  Sampling is warpAffine's convention, not the stretch form's half-pixel one: in float32, output
 * pixel (u, v) reads the frame at sx = xe + u * (We / out_w), sy = ye + v * (He / out_h), integer coordinates are pixel centres, bilinear
 * over the four neighbours, and a tap outside the frame contributes 0 (BORDER_CONSTANT; the edge is not replicated).  Normalisation,
 * bf16 store and out_c as pam_preprocess_crops.  antialias != 0: where We / out_w > 1 the taps are the integer positions within
 * max(We / out_w, 1) of sx (likewise in y), triangle weights, at most 24 per axis (the ones nearest the centre); a tap outside the frame
 * carries colour 0 but counts in the normaliser, so borders fade to black as the zero border does; where the scale is <= 1 the result is
 * the plain affine form's.  Like PIL's uint8 rounding above, warpAffine's uint8 rounding of the resampled image and its 1/32-pixel
 * fixed-point coordinates are not reproduced (float32 throughout), and there is no rotation.
 * PAM_E_ARG: as pam_preprocess_crops_ex / _flip, and for a NULL dev_eff_xywh or a box_scale that is not > 0.
 * pam_box_cs: the whole table in one tiny launch without cropping (n rows; a rank of the crop-sharded predict() crops its share only
 * while pam_pose_nms wants every row).  pam_box_cs_host: the same function in plain C++ on host memory.  The three tables agree bit for
 * bit (the library is built with -ffp-contract=off). */
int pam_preprocess_crops_affine(void* stream, int n, int n_total, int flip, const void* const* dev_frames, int frame_h, int frame_w,
                                const int32_t* dev_view_of, const float* dev_boxes, float box_scale, int out_h, int out_w, int out_c,
                                void* dev_out_bf16, int antialias, float* dev_eff_xywh);
int pam_box_cs(void* stream, int n, const float* dev_boxes, int out_w, int out_h, float box_scale, float* dev_eff_xywh);
int pam_box_cs_host(int n, const float* boxes, int out_w, int out_h, float box_scale, float* eff);
/* pam_head_decode_flip: pam_head_decode on the merged map of a plain and a mirrored crop, with the optional quarter-pixel offset.
 * feat: the feature batch of the forward above; crop i's plain features are row i, its mirrored features row flip_row0 + i (flip_row0 = n
 * in the layout of pam_preprocess_crops_flip).  P / F: the head's maps of the two (the FMA chain of pam_head_heatmaps, bit for bit).
 * flags, a bit set:
 *   PAM_FLIP_MERGE    M[j][y][x] = 0.5f * (P[j][y][x] + F[pair(j)][y][xs]): one float32 add, an exact halving; pair = the COCO left/right
 *                     swap 1<->2, 3<->4, ... 15<->16, 0<->0; xs = hm_w - 1 - x.  Without it M = P and the mirrored rows are never read.
 *   PAM_FLIP_SHIFT    (with MERGE only) xs = hm_w - x for x >= 1 and hm_w - 1 at x = 0: the official flipped[..., 1:] = flipped[..., :-1]
 *                     after the flip-back; column 0 keeps its own value.
 *   PAM_FLIP_QUARTER  the official get_final_preds offset: at an arg-max cell with 1 < px < hm_w - 1 and 1 < py < hm_h - 1 (both strict)
 *                     x += 0.25 sign(M[py][px+1] - M[py][px-1]), y likewise along the rows; a difference that is neither > 0 nor < 0
 *                     (zero, NaN) adds nothing.  The fractional cell goes through the box mapping of pam_decode_heatmaps (float64
 *                     arithmetic, one float32 rounding).  The official maxvals > 0 mask is not applied.
 * The arg-max (first maximum in flat order; a map with no value above -inf: cell 0, score -inf, no offset) and the score are those of M;
 * dev_heatmaps_or_null, when given, receives M (n, hm_h, hm_w, 17).  flags == 0: pam_head_decode itself, byte for byte.
 * dev_scratch: pam_head_decode_flip_scratch_bytes(n, hm_h, hm_w) bytes.  PAM_E_ARG: SHIFT without MERGE, unknown bits, MERGE with
 * flip_row0 < n, J != 17, C % 8 != 0, a null pointer. */
#define PAM_FLIP_MERGE 1
#define PAM_FLIP_SHIFT 2
#define PAM_FLIP_QUARTER 4
long long pam_head_decode_flip_scratch_bytes(int n, int hm_h, int hm_w);
int pam_head_decode_flip(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                         const float* bias, int J, int flags, float* dev_heatmaps_or_null, const int32_t* dev_view_of,
                         const int32_t* dev_slot_of, const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc,
                         void* dev_scratch);
/* pam_head_decode_dark: the DARK decode (Zhang et al., "Distribution-Aware Coordinate Representation for Human Pose Estimation", CVPR
 * 2020; the test protocol of the DARK-trained HRNet / Simple Baselines checkpoints) in the head pass: Gaussian blur, logarithm, one
 * Newton step of the log map's second-order Taylor expansion at the arg-max.  Arguments as pam_head_decode_flip; flags takes
 * PAM_FLIP_MERGE and PAM_FLIP_SHIFT under the rules there, and M is the map they define (M = P without MERGE).  blur_kernel = k, odd,
 * 9 <= k <= 17 (below 9 OpenCV uses fixed tap tables): R = (k - 1) / 2, sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8 (OpenCV's rule for
 * GaussianBlur(.., (k, k), 0): 2.0 at 11, 2.9 at 17), taps g[i] = exp(-(i - R)^2 / (2 sigma^2)) normalised to sum 1, in float64.
 *   1. (py, px) = arg-max of M, NOT of the blurred map (first maximum; nothing above -inf: cell 0); the score is M[py][px].
 *   2. The offset applies only where 1 < px < hm_w - 2 and 1 < py < hm_h - 2 (one cell tighter than PAM_FLIP_QUARTER: the second
 *      derivatives read +- 2); elsewhere the keypoint is the plain arg-max.
 *   3. B = blur(M): separable, rows first, then columns, float64 sums in ascending tap order, cells outside the map count as 0 (the
 *      official code frames the map with R zeros before cv2.GaussianBlur, so no reflected sample is ever read).
 *   4. L = log(max(B, 1e-10)) in float64 (a NaN is clamped as well).
 *   5. dx = 0.5 (L[py][px+1] - L[py][px-1]), dy alike; dxx = 0.25 (L[py][px+2] - 2 L[py][px] + L[py][px-2]), dyy alike;
 *      dxy = 0.25 (L[py+1][px+1] - L[py-1][px+1] - L[py+1][px-1] + L[py-1][px-1]).
 *   6. If dxx dyy - dxy^2 != 0: (ox, oy) = -H^-1 (dx, dy), keypoint (py + oy, px + ox).  Otherwise no offset.  Nothing clamps the offset.
 *   7. The box mapping of pam_decode_heatmaps (float64 arithmetic, one float32 rounding).
 * One deviation from the official code, which rescales B by max(M) / max(B) before the clamp: under the logarithm a positive scale is
 * an additive constant and drops out of every derivative, so it is left out (no whole-map maximum is needed and the maps stay out of
 * memory).  The results are equal whenever max(M) > 0, max(B) > 0 and no sampled B lies in (0, 1e-10 max(B) / max(M)] -- every map that
 * shows a joint (float64 check on planted blobs: 2e-14 cell).  On an all-negative map the official scale is negative and un-clamps the
 * map, an artefact; this entry point's definition is the scale-free one above.
 * dev_heatmaps_or_null receives M, as in pam_head_decode_flip.  dev_scratch: pam_head_decode_dark_scratch_bytes(n, hm_h, hm_w) bytes.
 * PAM_E_ARG: PAM_FLIP_QUARTER or unknown bits, an even or out-of-range blur_kernel, and what pam_head_decode_flip refuses.  n == 0: PAM_OK. */
long long pam_head_decode_dark_scratch_bytes(int n, int hm_h, int hm_w);
int pam_head_decode_dark(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                         const float* bias, int J, int flags, int blur_kernel, float* dev_heatmaps_or_null, const int32_t* dev_view_of,
                         const int32_t* dev_slot_of, const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc,
                         void* dev_scratch);
/* ---- the UDP protocol (Huang et al., "The Devil is in the Details: Delving into Unbiased Data Processing for Human Pose Estimation",
 * CVPR 2020; the test protocol of every public ViTPose checkpoint and of the HRNet / Simple Baselines "+UDP" ones) ----
 * The effective box (xe, ye, We, He) is the one above (UDP's _box2cs is the same function); only the pitch through it changes: crop and
 * heat-map are align-corners grids whose first and last points are the box's edges.
 * pam_preprocess_crops_udp: arguments, row layout, flip, antialias, out_c and dev_eff_xywh exactly as pam_preprocess_crops_affine.  In
 * float32, output pixel (u, v) reads the frame at sx = xe + u * (We / (out_w - 1)), sy = ye + v * (He / (out_h - 1)) (mmpose's
 * get_warp_matrix(0, 2c, size - 1, 200 s) inverted).  Everything else is the affine form's: integer coordinates are pixel centres,
 * bilinear over the four neighbours, a tap outside the frame contributes 0, a box with We == 0 is all zero, the antialias branch takes
 * the new pitch as its scale, the mirror rows are the column reversal bit for bit.  warpAffine's uint8 and fixed-point rounding are not
 * reproduced and there is no rotation.  PAM_E_ARG: as pam_preprocess_crops_affine, and for out_w < 2 or out_h < 2. */
int pam_preprocess_crops_udp(void* stream, int n, int n_total, int flip, const void* const* dev_frames, int frame_h, int frame_w,
                             const int32_t* dev_view_of, const float* dev_boxes, float box_scale, int out_h, int out_w, int out_c,
                             void* dev_out_bf16, int antialias, float* dev_eff_xywh);
/* pam_head_decode_udp: mmpose 0.x keypoints_from_heatmaps(use_udp=True, target_type='GaussianHeatmap') in the head pass: the UDP form
 * of DARK (post_dark_udp) and UDP's transform_preds.  Arguments as pam_head_decode_dark; flags takes PAM_FLIP_MERGE and PAM_FLIP_SHIFT
 * under the rules of pam_head_decode_flip (the UDP configs run the flip test without the shift) and M is the map they define.
 * blur_kernel = k is 0, or odd with 9 <= k <= 17; R, sigma and the float64 taps as in pam_head_decode_dark.
 *   1. (py, px) = arg-max of M, NOT of the blurred map (first maximum; nothing above -inf: cell 0); the score is M[py][px].
 *   2. blur_kernel == 0: no offset, step 8.
 *   3. B = GaussianBlur(M, (k, k), 0) with OpenCV's default border, BORDER_REFLECT_101: separable, rows first, then columns, float64
 *      sums in ascending tap order.  An index i outside [0, n) reads cell r(i): m = i mod 2 (n - 1) taken non-negative,
 *      r = m < n ? m : 2 (n - 1) - m (also where R >= n and the reflection bounces more than once).  No zero frame, no rescale.
 *   4. L = log(min(max(B, 0.001), 50)) in float64 (a NaN clamps to 0.001).
 *   5. L is read edge-replicated: sample (py + dy, px + dx) is taken at the coordinates clamped into the map.  There is NO inside rule:
 *      a winner on the border or in a corner takes the step too.
 *   6. Seven samples: the centre, x +- 1, y +- 1, (+1, +1) and (-1, -1).  dx = 0.5 (L[x+1] - L[x-1]), dy alike;
 *      dxx = L[x+1] - 2 L[0] + L[x-1], dyy alike (+- 1 and no 0.25, unlike DARK);
 *      dxy = 0.5 (L[+1,+1] - L[x+1] - L[y+1] + 2 L[0] - L[x-1] - L[y-1] + L[-1,-1]).
 *   7. H' = [[dxx + e, dxy], [dxy, dyy + e]], e = 2^-23 (np.finfo(np.float32).eps).  If det H' is non-zero and finite:
 *      (ox, oy) = -H'^-1 (dx, dy); otherwise no offset.  Nothing clamps the offset.
 *   8. UDP's transform_preds, float64 arithmetic with one float32 rounding: x = (double)xe + (px + ox) * ((double)We / (hm_w - 1)),
 *      y = (double)ye + (py + oy) * ((double)He / (hm_h - 1)), with (xe, ye, We, He) = dev_boxes[crop].  det and kp rows as in every decode.
 * Not reproduced: mmpose's float32 heat-map arithmetic (float64 here, from the float32 map) and the CombinedTarget offset-map decode.
 * dev_heatmaps_or_null receives M, as in pam_head_decode_flip.  dev_scratch: pam_head_decode_udp_scratch_bytes(n, hm_h, hm_w) bytes (-1
 * for a refused shape).  PAM_E_ARG: hm_w < 2 or hm_h < 2, PAM_FLIP_QUARTER or unknown bits, a blur_kernel that is neither 0 nor odd in
 * [9, 17], and what pam_head_decode_flip refuses.  n == 0: PAM_OK. */
long long pam_head_decode_udp_scratch_bytes(int n, int hm_h, int hm_w);
int pam_head_decode_udp(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                        const float* bias, int J, int flags, int blur_kernel, float* dev_heatmaps_or_null, const int32_t* dev_view_of,
                        const int32_t* dev_slot_of, const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc,
                        void* dev_scratch);
int pam_decode_heatmaps(void* stream, int n, const float* dev_heatmaps, int nchw, int hm_h, int hm_w,
                        const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes,
                        int max_dets, double* dev_det, float* dev_kp_xyc /*optional n*17*3 (x,y,conf) or NULL*/);
/* measurement aid, not part of the path: one wave spins `microseconds` and writes {delta shader cycles (s_memtime), delta 100 MHz
 * ticks (s_memrealtime)} to dev_out2 -> shader clock [MHz] = 100 * out[0] / out[1] at that point of the stream (bench.py records it
 * right before and right after the timed region). */
int pam_clock_probe(void* stream, unsigned long long* dev_out2, int microseconds);

/* ---- HRNet conv stack (a1) as hand-written MFMA kernels -------------------------------------------------------
 * pam_conv2d_nhwc_bf16: NHWC bf16 convolution (KH,KW in {1,3}; stride 1/2; Cin % 8 == 0; Cout % 48 == 0, % 64 == 0 or % 32 == 0) as an
 * implicit GEMM on v_mfma_f32_16x16x32_bf16 with fused epilogue out = act(conv + bias [+ residual]); `relu` is the activation
 * code: 0 linear, 1 ReLU, 2 leaky ReLU (slope 0.1, Darknet), 3 mish (YOLOv4: in float32 on conv + bias, e = expf(x), n = e*e + 2e,
 * x <= -0.6f ? x * (n / (n + 2)) : x - 2 * (x / (n + 2)); carried by the Darknet-only instantiations: the G = 1 forms of k_conv_igemm /
 * k_conv3x3s and the mish forms of k_conv_stem (stride 1) / k_conv_gs below; never on k_conv3x3);
 * + 4 = add the residual AFTER the activation (Darknet shortcut).  w_packed is
 * [Cout][Kpad] bf16, k = (ky, kx, cin) flattened, zero-padded to Kpad = roundup(KH*KW*Cin, 64); bias float32 or NULL;
 * residual NHWC bf16 of the output shape or NULL.  tile_cfg: -1 = choose automatically (w_img in the layout pam_conv3x3_layout() announces
 * at call time), -3 / -4 = the same with the layout of w_img STATED by the caller (-3 streamed: k_conv3x3s or PAM_E_ARG; -4 classic),
 * -2 = the classic kernels (k_conv3x3 /
 * k_conv_igemm) with automatic tiles, 0..7 = one k_conv_igemm tile shape (Cout a multiple of 32 only: 0 / 2), 8 = the streamed implicit GEMM k_conv_gs (activation codes 0 / 1).  w_img (optional, 3x3 stride-1 layers
 * with Cin in {48,64,96,128,192,256,384,512}, or 32 -> 32): the same weights pre-packed as per-chunk LDS images [Cout/BN][Cin/CK][BN][9*CK + pad] (BN =
 * pam_conv3x3_slab(H, W, Cin, Cout); CK = 48 if Cin == 48, 64 if Cin >= 192, else 32; row pitch 864 / 1184 / 608 bytes;
 * row j*16 + q of a slab, q < 16, j < BN/16, holds output channel 4*(BN/16)*(q >> 2) + 4*j + (q & 3) of that slab) for the
 * rows-in-LDS kernel k_conv3x3; for a stem layer (Cin 8, Cout 32 or 64, 3x3, stride 1 or 2, pad 1; Cout 32 is accepted only
 * here) w_img is instead the MFMA A fragments of k_conv_stem, [j < Cout/16][ky < 3][lane < 64][8] bf16: lane l = input channels
 * 0..7 of tap (ky, kx = l >> 4; zero for l >= 48) of output channel (Cout/4)*((l & 15) >> 2) + 4*j + (l & 3).  NULL = generic kernel.
 * pam_upsample_add_nhwc_bf16: the HRNet fuse-layer sum out = [relu](base + sum_t nearest_upsample(term_t, 2^shift_t)). */
int pam_conv2d_nhwc_bf16(void* stream, const void* in, const void* w_packed, const void* w_img, const float* bias,
                         const void* residual, void* out, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                         int stride, int pad, int relu, int tile_cfg);
/* the same with channel-sliced operands, for the merged fuse-layer convolutions: the input pixels are in_cstride channels apart
 * (`in` points at the first of the Cin channels read; 0 = Cin), and the activation applies only to output channels >= relu_from
 * (multiple of 16; 0 = all).  Either option selects the generic kernel. */
int pam_conv2d_nhwc_bf16_ex(void* stream, const void* in, const void* w_packed, const void* w_img, const float* bias,
                            const void* residual, void* out, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                            int stride, int pad, int relu, int tile_cfg, int in_cstride, int relu_from);
/* output channels per workgroup slab (BN) that k_conv3x3 uses for a layer shape; weight images must be packed with it */
int pam_conv3x3_slab(int H, int W, int Cin, int Cout);
/* 0: w_img of this layer is the classic per-chunk image described above; BN > 0: the layer runs on the streamed kernel k_conv3x3s
 * (Cin 192 / 384 at tile_cfg == -1) with slabs of BN output channels and w_img must be [Cout/BN][Cin/32][9 taps][BN rows][4][8]
 * bf16: chunk c, tap t, row r (same row -> channel rule as above) holds input channels 32*c + 8*g .. + 8 of that tap in its 16-byte
 * piece g ^ ((r >> 1) & 2).  tile_cfg == -2 forces the classic kernel (and the classic image) for such a layer.  BN > 0 is only
 * returned for shapes the streamed kernel is instantiated for (64-channel slabs for Cin 64 / 192 / 384, the 48-channel slab for
 * 256 -> 48); the streamed kernel takes activation codes 0 / 1 only, so a layer with a Darknet code (relu > 1) must be packed in the
 * classic layout and called with tile_cfg == -2 (tile_cfg == -1 with a streamed image and relu > 1 returns PAM_E_ARG). */
int pam_conv3x3_layout(int H, int W, int Cin, int Cout);
/* the same with the 96 -> 96 layers' choice stated: c96_slab 0 = they stay on k_conv3x3 (the answer above), 48 = streamed with slabs
 * of 48 output channels (the only streamed slab width instantiated for these layers; any other value answers as 0).  The caller packs
 * the image for the slab returned and says so at the launch: tile_cfg -5 of pam_conv2d_nhwc_bf16_ex, which otherwise behaves like -3
 * (streamed layout stated; -4 = classic layout stated). */
int pam_conv3x3_layout_ex(int H, int W, int Cin, int Cout, int c96_slab);
/* Darknet's 3x3 stride-1 layers (activation codes > 1: leaky, shortcut added after the activation) on the streamed kernel: the slab
 * width (64 for Cin 128, 32 for Cin 256 / 512) when the library has a general-activation instantiation for the shape (Cout % 64 == 0,
 * rows that fit the patch), else 0.  The caller then packs the streamed image for slabs of that width and launches with tile_cfg -7 (any other tile_cfg keeps such layers on
 * the classic kernel and image). */
int pam_conv3x3_layout_gen(int H, int W, int Cin, int Cout);
/* round 5: 192- / 384-channel ReLU / linear 3x3 layers with 32-channel slabs (tile_cfg -8 of pam_conv2d_nhwc_bf16_ex; w_img packed as
 * above for slabs of 32): twice the workgroups, each half as long -- for forwards of a few crops, whose launches are as long as one
 * workgroup.  Same arithmetic and summation order as the 64-channel-slab form (bit-identical).  > 0: supported, the slab width (32). */
int pam_conv3x3_layout_small(int H, int W, int Cin, int Cout);
/* which kernel the calling thread's last pam_conv2d_nhwc_bf16[_ex] call launched (labels for per-kernel profiles) */
#define PAM_CONV_KERNEL_IGEMM 0   /* k_conv_igemm */
#define PAM_CONV_KERNEL_3X3   1   /* k_conv3x3   */
#define PAM_CONV_KERNEL_3X3S  2   /* k_conv3x3s  */
#define PAM_CONV_KERNEL_GS    3   /* k_conv_gs   */
#define PAM_CONV_KERNEL_STEM  4   /* k_conv_stem */
int pam_conv_last_kernel(void);
/* which instantiation of that kernel it launched, a decimal code whose fields are the kernel's template parameters:
 *   PAM_CONV_KERNEL_IGEMM  G*1000000 + BM*1000 + BN       G = 1: general-activation epilogue (codes > 1); BM x BN = pixel x channel tile
 *   PAM_CONV_KERNEL_3X3    Cin*10 + NTW                   output-channel slab 16*NTW
 *   PAM_CONV_KERNEL_3X3S   G*100000 + Cin*100 + NTW*10 + MT   G = 1: general-activation form (tile_cfg -7); slab 16*NTW; MT M tiles per wave
 *   PAM_CONV_KERNEL_GS     NBUF*1000000 + BM*1000 + M*500 + 16*NTW    chunk ring depth, pixel tile, M = 1: the mish form (k_conv_gs_mish), output-channel slab
 *   PAM_CONV_KERNEL_STEM   M*1000 + S*100 + Cout          M = 1: the mish form (k_conv_stem_mish, stride 1); stride 1 / 2, 32 or 64 output channels
 * Kernel and form are recorded together, by the launcher, from the launched kernel's own template parameters. */
int pam_conv_last_form(void);
/* Which kernel and form (the two codes above) pam_conv2d_nhwc_bf16_ex would launch for these integer arguments and pointers (has_* = 1
 * where the call passes a non-NULL in / w_packed / w_img / residual / out): the library's own choice, asked without launching.  Returns
 * what the call would return before it launches: PAM_OK with *kernel and *form written, or PAM_E_ARG (a refused call, or a NULL output)
 * with both left alone.  Pure integer arithmetic: touches no device and works on a machine without a GPU. */
int pam_conv_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, int tile_cfg, int in_cstride,
                  int relu_from, int has_in, int has_w_packed, int has_w_img, int has_residual, int has_out, int32_t* kernel, int32_t* form);
/* diagnostic builds only: device buffer (64 x uint64 per workgroup) for k_conv3x3's s_memtime stamps, used when tile_cfg = 100 + 64 */
int pam_conv_debug_stamps(void* dev_buf);
int pam_upsample_add_nhwc_bf16(void* stream, const void* base, int n_terms, const void* const* terms,
                               const int32_t* shifts, void* out, int N, int H, int W, int C, int relu);
/* the same with terms that are channel slices of wider tensors: term_cstrides[t] = channels between pixels of term t (NULL / 0 = C) */
int pam_upsample_add_nhwc_bf16_ex(void* stream, const void* base, int n_terms, const void* const* terms, const int32_t* shifts,
                                  const int32_t* term_cstrides, void* out, int N, int H, int W, int C, int relu);

/* ---- fused HRNet BasicBlock (row a1; stands inside the absent HRNet backend behind /root/reference/src/ivclabpose.py:210).
 * out = ReLU(conv3x3(ReLU(conv3x3(in) + b1)) + b2 + in), NHWC bf16, C -> C -> C, stride 1, pad 1, BatchNorm folded; the intermediate
 * never leaves LDS.  ONE launch per tensor with 2-D items of tile_rows x tile_cols output positions (csrc/pam_block2.hip), all
 * operands fetched by LDS-DMA; C = 32, 48 or 96.  pam_basic_block2_tile writes the {rows, cols} the library would pick for N x H x W (whole rounds of 256
 * workgroups first, then the least work per item); tile_rows / tile_cols <= 0 in the launch = that choice.  in != out.
 * C = 48 (k_bblock2_48): BOTH weight sets resident in LDS beside a 75 KB input tile, no barrier inside the K loops.  Limits:
 *   (rows + 4)(cols + 4) <= 800, (rows + 2)(cols + 4) <= 768, rows (cols + 2) <= 640.
 *   wpack (1 024 + 86 016 bytes): [float32 bias: conv1's 48, conv2's 48, zero padding to 1 KiB][conv1's 14 k-step images][conv2's 14]; a
 *   k-step = 32 K elements, K = flattened (tap, cin) index padded with zeros to 14*32; a k-step image = [48 rows][64 bytes = 4 pieces
 *   of 8 bf16]: row j*16 + q = output channel 8*(q >> 2) + 4*j + (q & 3) for j < 2 and 32 + 4*(q >> 2) + (q & 3) for j = 2, and
 *   physical piece p of row R holds K elements 8*(p ^ s) .. + 7 of the k-step with s = (0,2,3,1)[(R%16) >> 2] (LDS bank swizzle).
 *   Results are bit-identical to two pam_conv2d_nhwc_bf16 calls (same K order per output element).
 * C = 96 (k_bblock2_96<3,2>): the input tile resident (chunk-major, 3 x 32 channels), the weights of both convolutions
 *   streamed through a ring of six k-step images (twelve while the tile's (rows + 4)(cols + 4) slots, rounded up to 16, stay <= 448).
 *   Limits of the one instantiation shipped (<3,2>): (rows + 4)(cols + 4) <= 640, (rows + 2)(cols + 4) <= 384, rows (cols + 2) <= 256.
 *   wpack (1 024 + 331 776 bytes): [float32 bias 96 + 96, padded to 1 KiB][54 k-step images of [96 rows][64 bytes]] in the order (conv,
 *   chunk of 32 input channels, tap); row j*16 + q = output channel 24*(q >> 2) + 4*j + (q & 3); physical 16-byte piece p of row r
 *   holds the chunk's input channels 8*(p ^ ((r >> 1) & 2)) .. + 7.  The residual enters the sum before the products (as in the
 *   streamed convolution kernel): equal to the two-launch path to within the last bf16 bit.
 * C = 32 (k_bblock2_32, csrc/pam_block32.hip; HRNet-W32): both weight sets resident in LDS (2 x 18 KB), no barrier inside the K loops.
 *   Limits: (rows + 2)(cols + 4) <= 768, rows (cols + 2) <= 640, (rows + 4)(cols + 4) <= 1968.  Activation slots of 64 bytes in LDS with
 *   physical piece p of slot s holding channels 8*(p ^ ((s >> 2) & 3)) .. + 7 (conflict-free ds_read_b128 at every tap offset).
 *   wpack (1 024 + 36 864 bytes): [float32 bias: conv1's 32, conv2's 32, zero padding to 1 KiB][conv1's 9 k-step images][conv2's 9]; k-step
 *   t = tap t (ky * 3 + kx), its 32 K elements = the 32 input channels; a k-step image = [32 rows][64 bytes = 4 pieces of 8 bf16]: row
 *   j*16 + q = output channel 8*(q >> 2) + 4*j + (q & 3), physical piece p of row R holds input channels 8*(p ^ ((R >> 2) & 3)) .. + 7.
 *   Results are bit-identical to two pam_conv2d_nhwc_bf16 calls on k_conv3x3<32> (same K order per output element). */
int pam_basic_block2_tile(int C, int N, int H, int W, int32_t* out2);
int pam_basic_block2_nhwc_bf16(void* stream, const void* in, const void* wpack, void* out, int N, int H, int W, int C,
                               int tile_rows, int tile_cols);

/* ---- the pointwise tail of a layer1 Bottleneck as ONE launch (row a1; csrc/pam_pw.hip) ------------------------------------------
 * X = ReLU(W3 . y2 [+ Wd . x0] + bias3 [+ residual]);  y1 = ReLU(W1 . X + bias1)   per pixel, NHWC bf16:
 * y2 (n_pixels x 64): the block's 3x3 output; x0 (n_pixels x 64, or NULL): the first block's input, whose 1x1 downsample convolution is
 * a second K range of the same product (bias3 then = conv3's + the downsample's); residual (n_pixels x 256, or NULL; not with x0);
 * out_x (n_pixels x 256); w1_img / bias1 / out_y1 (n_pixels x 64): the NEXT block's conv1, or all NULL.  HRNet-W48's widths only.
 * w3_img [S][256][64] bf16 (S = 1, or 2 with x0): chunk c = K source c; row 64 sl + 16 jt + qq (qq < 16) = output channel
 *   64 sl + 16 (qq >> 2) + 4 jt + (qq & 3); the row's 16-byte piece at position p holds K values 8 q .. 8 q + 7, q = p ^ ((row >> 1) & 7).
 * w1_img [4][64][64] bf16: chunk sl = input channels 64 sl .. + 63; row 16 jt + qq = output channel 16 (qq >> 2) + 4 jt + (qq & 3);
 *   piece p holds, with q = p ^ ((row >> 1) & 7), h = q >> 2, g = q & 3, the input channels 64 sl + 16 g + 8 h .. + 7.
 * tile_cfg: 16-pixel tiles per wave tile (1..3), <= 0 = automatic.  replaces: conv3 + bn3 + residual + relu and the next conv1 + bn1 +
 * relu of the official Bottleneck (the HRNet backend is absent from the reference: call sites /root/reference/src/ivclabpose.py:131-132,210). */
/* Round 4: HRNet's stem and the first Bottleneck's conv1 as ONE launch (csrc/pam_stem.hip):
 *   c1 = ReLU(conv3x3 s2 p1 (in; 8 -> 64) + bias1), x0 = ReLU(conv3x3 s2 p1 (c1; 64 -> 64) + bias2), y1 = ReLU(conv1x1 (x0; 64 -> 64) + biasp);
 * c1 stays in LDS.  in (N, H, W, 8) bf16 NHWC, out_x0 / out_y1 (N, H2, W2, 64) with H1 = (H - 1) / 2 + 1, H2 = (H1 - 1) / 2 + 1 (W alike).
 * w1frag: the 8 -> 64 layer's w_img of pam_conv2d_nhwc_bf16 (k_conv_stem's A fragments, [4][3][64 lanes][8]); wp_img / biasp:
 * pam_pointwise64_relu_nhwc_bf16's; w2img [9 taps][64 rows][64 K] bf16: row 16 j + q of a tap = output channel
 * 32 (j >> 1) + 8 (q >> 2) + 4 (j & 1) + (q & 3), the row's 16-byte piece at position p holds input channels 8 c .. 8 c + 7 with
 * c = p ^ ((q >> 1) & 7).  Results are bit-identical to the three launches it replaces (pam_conv2d_nhwc_bf16 twice, then
 * pam_pointwise64_relu_nhwc_bf16).  replaces: conv1/bn1/relu, conv2/bn2/relu and layer1[0].conv1/bn1/relu of the official pose_hrnet (the
 * HRNet backend is absent from the reference: call sites /root/reference/src/ivclabpose.py:131-132,210). */
int pam_stem_fused_nhwc_bf16(void* stream, const void* in, const void* w1frag, const float* bias1, const void* w2img, const float* bias2,
                             const void* wp_img, const float* biasp, void* out_x0, void* out_y1, int N, int H, int W);
/* Round 4: the 3x3 convolution of a layer1 Bottleneck and its pointwise tail as ONE launch (csrc/pam_bneck.hip):
 *   y2 = ReLU(conv3x3 s1 p1 (y1; 64 -> 64) + bias2), then pam_bottleneck_tail_nhwc_bf16's X = ReLU(W3 . y2 + bias3 + residual) and
 *   y1' = ReLU(W1 . X + bias1) (w1_img / bias1 / out_y1 all NULL: no second product); y2 never leaves the registers.
 * y1 (N, H, W, 64), residual / out_x (N, H, W, 256), out_y1 (N, H, W, 64), bf16 NHWC.  Exactly one of residual and x0 (N, H, W, 64: the
 * FIRST block's input, whose 1x1 downsample convolution is the second K source of w3_img, as in pam_bottleneck_tail_nhwc_bf16) is given.
 * w2img: the [9 taps][64 rows][64 K] image of pam_stem_fused_nhwc_bf16; w3_img (one K source, two with x0) / w1_img:
 * pam_bottleneck_tail_nhwc_bf16's.  Results are bit-identical to
 * pam_conv2d_nhwc_bf16 (streamed 3x3 kernel) followed by pam_bottleneck_tail_nhwc_bf16.  replaces: conv2/bn2/relu, conv3/bn3 + residual +
 * relu and the next conv1/bn1/relu of the official Bottleneck (call sites /root/reference/src/ivclabpose.py:131-132,210). */
int pam_bottleneck_fused_nhwc_bf16(void* stream, const void* y1, const void* x0, const void* residual, const void* w2img,
                                   const float* bias2, const void* w3_img, const float* bias3, const void* w1_img, const float* bias1,
                                   void* out_x, void* out_y1, int N, int H, int W);
/* ---- PoseResNet (Simple Baselines) layers of its own (csrc/pam_resnet.hip; executor: hrnet_hip.HipPoseResNet) ----------------
 * pam_resnet_stem_nhwc_bf16: conv 7x7 stride 2 pad 3 (8 -> 64 channels) + bias + ReLU, then max-pool 3x3 stride 2 pad 1, in ONE launch (the
 * H/2 map stays in LDS).  in (N, H, W, 8) bf16 NHWC (RGB + 5 zero channels: pam_preprocess_crops(out_c = 8)); out (N, Hp, Wp, 64) bf16 NHWC
 * with Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1 (W alike).  wfrag [4 n-tiles j][7 ky][2 k-steps s][64 lanes][8] bf16: lane l holds, for
 * output channel 16 ((l & 15) >> 2) + 4 j + (l & 3), input channels 0 .. 7 of tap (ky, kx = 4 s + (l >> 4)); kx = 7 is zero.  bias [64] float32.
 * Constraints: N >= 1, H, W >= 2, Wc <= 192, N H W 16 < 2^31 and N Hp Wp 128 < 2^31 (32-bit offsets).  PAM_E_ARG otherwise (null pointer
 * included), PAM_E_HIP on a launch error. */
int pam_resnet_stem_nhwc_bf16(void* stream, const void* in, const void* wfrag, const float* bias, void* out, int N, int H, int W);
/* pam_deconv4x4s2_nhwc_bf16: ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1, output_padding 0) + bias [+ ReLU when relu = 1] in one launch
 * for all four output parities.  in (N, H, W, Cin) bf16 NHWC -> out (N, 2H, 2W, Cout) bf16 NHWC; bias [Cout] float32 (BN folded).
 * wimg: Cin Cout 16 bf16, [parity p = 2 py + px][slab s = Cout / 64][k-step c = Cin / 32][tap t = 2 ty + tx][n-tile j = 4][lane 64][8]: lane l
 * holds output channel 64 s + 16 ((l & 15) >> 2) + 4 j + (l & 3) and input channels 32 c + 8 (l >> 4) .. + 7 of kernel tap (ky, kx) with
 * ky = (1, 3)[ty] for py = 0 and (2, 0)[ty] for py = 1 (kx alike from px, tx): output (2 m + py, 2 k + px) reads input (m + dy, k + dx) with
 * dy = (0, -1)[ty] / (0, +1)[ty].  Constraints: Cin % 32 == 0, Cout % 64 == 0, W <= 128, relu in {0, 1}, N H W Cin 2 < 2^31 and
 * N 4 H W Cout 2 < 2^31 (32-bit offsets).  PAM_E_ARG otherwise (null pointer included), PAM_E_HIP on a launch error. */
int pam_deconv4x4s2_nhwc_bf16(void* stream, const void* in, const void* wimg, const float* bias, void* out, int N, int H, int W,
                              int Cin, int Cout, int relu);
/* ---- ViTPose token kernels (csrc/pam_vit.hip; executor: hrnet_hip.HipViTPose) ---------------------------------------------------
 * Activations are bf16; a token tensor of M = B T rows and D channels is the NHWC tensor (B, 16, 12, D).  Biases, LayerNorm's gamma / beta
 * and the position table are float32.  Every entry point answers PAM_E_ARG on a null pointer (residual excepted) or a shape outside
 * the constraints below, PAM_E_HIP on a launch error.
 * Linear weight image (packing.PackedLinear), N K bf16: [slab s = N / 64][k-step c = K / 32][n-tile j = 4][lane 64][8]: lane l holds output
 * channel 64 s + 16 ((l & 15) >> 2) + 4 j + (l & 3) and input channels 32 c + 8 (l >> 4) .. + 7.
 * pam_vit_linear_bf16: out = bf16(act(x . w^T + bias) [+ residual]), x (M, K), out and residual (M, N); act 0 = linear, 1 = exact GELU
 * 0.5 v (1 + erff(v 0.70710678f)) in float32; a residual only with act 0.  float32 accumulation (v_mfma_f32_16x16x32_bf16), one bf16
 * rounding.  Constraints: K % 64 == 0, N % 64 == 0, M >= 1; frontier: M K 2 < 2^31 and M N 2 < 2^31 bytes (32-bit buffer offsets), N <= 128 * 65535. */
int pam_vit_linear_bf16(void* stream, const void* x, const void* w, const float* bias, const void* residual, void* out, int M, int K, int N,
                        int act);
/* pam_vit_patch_embed_bf16: Conv2d(3, D, 16, stride 16, padding 2) of the crop kernel's (N, H, W, 8) bf16 output + the folded position
 * table: out[n][t][d] = bf16(sum + pos_bias[t][d]), t = ty (W / 16) + tx, out (N, T = H W / 256, D); pos_bias (T, D) float32 =
 * pos[t + 1] + pos[0] + bias, folded by the host.  Taps in the 2-pixel border outside the crop read zero.  The weights are packed for
 * ALL 8 channels of a pixel (channels 3 .. 7 zero): the linear image above with K = 2048 in the order (ky, kx, channel).
 * Constraints: H % 16 == 0, W % 16 == 0, D % 64 == 0; frontier: N H W 16 < 2^31 and N T D 2 < 2^31 bytes, D <= 128 * 65535. */
int pam_vit_patch_embed_bf16(void* stream, const void* x8, const void* w, const float* pos_bias, void* out, int N, int H, int W, int D);
/* pam_vit_layernorm_bf16: out = bf16((x - mean) / sqrt(var + eps) * gamma + beta) per row of D channels; mean and the variance of the
 * centred values in float32 over the row held in registers, one bf16 rounding.  Constraints: D % 64 == 0, D <= 2048, M >= 1, eps >= 0
 * (offsets are 64-bit: no frontier below M = 2^31). */
int pam_vit_layernorm_bf16(void* stream, const void* x, const float* gamma, const float* beta, void* out, int M, int D, float eps);
/* pam_vit_attention_bf16: softmax(Q K^T / 8) V per (crop, head) over all T keys, head dimension 64: qkv (B, T, 3, heads, 64), out
 * (B, T, heads 64).  Scores in float32 (scale 0.125 applied in float32), the row maximum subtracted, expf, P rounded to bf16 for the
 * P V product -- as two bf16 terms, the rounding and the rounding of its remainder, so that P's error stays below the 2^-9 sum p |v|
 * the kernel is tested against (one bf16 rounding alone is up to 2^-8) --, the result divided by the float32 sum of the unrounded
 * exponentials, one bf16 rounding at the store.  Constraints: T % 16 == 0,
 * 16 <= T <= 192, B <= 65535, heads <= 65535 (grid dimensions; offsets are 64-bit). */
int pam_vit_attention_bf16(void* stream, const void* qkv, void* out, int B, int T, int heads);
/* y = ReLU(W . x + bias), 64 -> 64 channels, pointwise (the first Bottleneck's conv1 on the stem output): w_img [64 rows][64 K] bf16, row
 * 16 jt + qq = output channel 16 (qq >> 2) + 4 jt + (qq & 3), natural K order, the row's 16-byte piece at position p holds K values
 * 8 q .. 8 q + 7 with q = p ^ ((row >> 1) & 7). */
int pam_pointwise64_relu_nhwc_bf16(void* stream, const void* in, const void* w_img, const float* bias, void* out, long long n_pixels);
/* the same stream with the activation stated: act 1 = ReLU, 2 = leaky ReLU of slope 0.1 (Darknet's 64 -> 32 pointwise layer, its 32 filters
 * zero-padded to 64, at 208 x 208) */
int pam_pointwise64_act_nhwc_bf16(void* stream, const void* in, const void* w_img, const float* bias, void* out, long long n_pixels, int act);
int pam_bottleneck_tail_nhwc_bf16(void* stream, const void* y2, const void* x0, const void* residual, const void* w3_img,
                                  const float* bias3, const void* w1_img, const float* bias1, void* out_x, void* out_y1,
                                  long long n_pixels, int tile_cfg);

/* ---- round 5: the fuse layers of an HR module (row a1; hrnet_model.py, HighResolutionModule -- stands inside the absent HRNet backend behind
 * /root/reference/src/ivclabpose.py:210): every output i of a module is ReLU(x_i + strided-convolution chains from the finer branches +
 * up-sampled 1x1 convolutions of the coarser ones).
 *
 * pam_conv3x3s2_c48_nhwc_bf16 (csrc/pam_down.hip, k_down48): out = [ReLU on channels >= relu_from](conv3x3 stride 2 pad 1 (in) + bias
 * [+ res]) for Cin = 48: the input patch of a tile of output positions resident in LDS (columns stored by parity), the output channels
 * walked in 48-channel slabs whose weights are resident and double-buffered.  in: (N, H, W) pixels of in_cstride channels (the first 48
 * are read: a channel slice of a wider tensor is fine); out / res: (N, Ho, Wo) pixels of out_cstride / res_cstride channels, Ho = (H - 1)
 * / 2 + 1; Cout % 48 == 0.  wpack: Cout / 48 slab images of 43 008 bytes, slab s = output channels 48 s .. + 47 in the layout of ONE
 * convolution of pam_basic_block2_nhwc_bf16's C = 48 image ([14 k-steps][48 rows][64 bytes], see there).  tile_rows / tile_cols <= 0 and
 * slab_groups <= 0: the library's choice (pam_conv3x3s2_c48_tile writes {rows, cols, groups}); slab_groups = workgroups an item's slabs
 * are spread over (divides Cout / 48).  Results are bit-identical to pam_conv2d_nhwc_bf16 (same K order per output element).
 *
 * pam_fuse_sum_nhwc_bf16 (csrc/pam_fuse.hip: one front, two kernels, k_fuse_sum and k_fuse_sum_lds): out = [ReLU](base + sum_t plain_t + sum_s nearest_up_{2^shift_s}(W_s . src_s +
 * bias_s)): base / out / plain_t (N, H, W, C) NHWC bf16, C in {48, 96, 192} (plain_t may be channel slices: plain_cstrides, NULL = C);
 * src_s (N, H >> shift_s, W >> shift_s, up_channels[s]) with ascending shifts, up_channels % 32 == 0, H and W multiples of 2^shift;
 * up_wimg[s]: the 1x1 weights (C x up_channels[s]) as MFMA A fragments, bf16 [C / 16][up_channels / 32][64 lanes][8]: lane l of fragment
 * (j, ks) holds W[16 j + (l & 15)][32 ks + 8 (l >> 4) .. + 7]; up_bias[s]: float32 [C] or NULL.  n_plain <= 2, 1 <= n_up <= 3.  The k loops
 * are unrolled per source, so up_channels[s] must be C << up_shifts[s] and (C, shifts) a row of the table FUSE_COMBOS of
 * csrc/pam_fuse_plan.hpp: (1), (1, 2), (1, 2, 3) for C = 48, (1), (1, 2), (2) for C = 96, (1) for C = 192 (every HRNet fuse layer;
 * anything else: PAM_E_ARG at every size, looked up before a kernel is chosen).  k_fuse_sum: one small workgroup (C / 16 waves, each with its
 * channel tile's 1x1 weights of all sources in registers) per unit of 16 pixels of an anchor level L, i.e. 16 blocks of 2^L x 2^L output
 * pixels; the products never reach HBM; sum order = base, plain terms, up terms (the order of pam_upsample_add_nhwc_bf16 with the terms in
 * branch order; the three kernels share one statement of it, sum8_* of csrc/pam_kernel.hpp).  tile_a, tile_b and max_workgroups are
 * HINTS, any value gives the same results: tile_a > 0 asks for the anchor level
 * L = tile_a (clamped to min(2, coarsest shift)); tile_b is not used.  With tile_a <= 0 the library chooses the level and, for the sizes
 * where it is still the faster one (C = 192 outside 65 .. one unit per CU, C = 96 under two sources above 768 units), the earlier
 * persistent kernel k_fuse_sum_lds (one workgroup per CU at most, weights in LDS), which alone honours max_workgroups > 0 as a cap.
 * Results are bit-identical to pam_conv2d_nhwc_bf16 (1x1) per source followed by pam_upsample_add_nhwc_bf16.
 * pam_fuse_sum_plan: the same decision (csrc/pam_fuse_plan.hpp) asked without a launch: PAM_OK exactly when pam_fuse_sum_nhwc_bf16 would
 * accept these integers with every pointer given and plain_cstrides NULL, else PAM_E_ARG (a NULL out8 too) with out8 left alone.
 * out8 = {kernel (1 = k_fuse_sum, 2 = k_fuse_sum_lds), L (0 for kernel 2), log2 of the unit's rows | tile rows TA of the coarsest
 * source, log2 of the unit's columns | TB, units | tiles per image down, across, workgroups, dynamic LDS bytes}.  n_cu <= 0: the current
 * device's compute units (256 where there is no device).  Touches no device memory and works on a machine without a GPU. */
int pam_conv3x3s2_c48_tile(int N, int H, int W, int Cout, int32_t* out3);
/* the same convolution for Cin = 96 / 192 (k_down_s: the streamed 3x3 kernel with a stride-2, parity-planar patch; no residual).
 * pam_conv3x3s2_slab: the slab width BN (64 or 48 output channels) the library takes for this shape, 0 = not taken (generic kernel);
 * w_img: the streamed 3x3 image of pam_conv2d_nhwc_bf16 for that BN ([Cout / BN][Cin / 32][9 taps][BN rows][4 pieces of 8 bf16]: row
 * j*16 + q of a slab = its channel 4*(BN/16)*(q >> 2) + 4*j + (q & 3), physical piece p of row r = the chunk's input channels
 * 8*(p ^ ((r >> 1) & 2)) .. + 7).  relu_from % 16 == 0.  Equal to pam_conv2d_nhwc_bf16 up to the summation order (K walked chunk by
 * chunk of 32 input channels instead of tap by tap): within one bf16 rounding of the fp32 result. */
int pam_conv3x3s2_slab(int H, int W, int Cin, int Cout);
int pam_conv3x3s2_nhwc_bf16(void* stream, const void* in, int in_cstride, const void* w_img, const float* bias, void* out, int N, int H,
                            int W, int Cin, int Cout, int relu, int relu_from);
int pam_conv3x3s2_c48_nhwc_bf16(void* stream, const void* in, int in_cstride, const void* wpack, const float* bias, const void* res,
                                int res_cstride, void* out, int out_cstride, int N, int H, int W, int Cout, int relu, int relu_from,
                                int tile_rows, int tile_cols, int slab_groups);
int pam_fuse_sum_nhwc_bf16(void* stream, const void* base, int n_plain, const void* const* plain, const int32_t* plain_cstrides, int n_up,
                           const void* const* up_src, const int32_t* up_shifts, const int32_t* up_channels, const void* const* up_wimg,
                           const float* const* up_bias, void* out, int N, int H, int W, int C, int relu, int tile_a, int tile_b,
                           int max_workgroups);
int pam_fuse_sum_plan(int N, int H, int W, int C, int n_plain, int n_up, const int32_t* up_shifts, const int32_t* up_channels,
                      int tile_a, int tile_b, int max_workgroups, int n_cu, int32_t* out8);

/* ---- round 5: device-side ordering of the forward's branch streams (csrc/pam_sync.hip; the module-end exchange of hrnet_model.py, HighResolutionModule inside
 * the absent HRNet backend, /root/reference/src/ivclabpose.py:210).  pam_flag_signal: one agent-scope atomic add on *dev_counter behind
 * everything already queued on `stream`.  pam_flag_gate: [arrive != 0: first the same add, then] `stream` goes on once *dev_counter >= target (one wave polls; the launches that
 * follow on the stream see what the signalling streams' earlier kernels wrote); after *dev_max_us microseconds (a device word read when
 * the gate starts: the bound of a captured gate can be changed between replays) it sets *dev_err = 1 and lets the stream go on
 * regardless -- the caller checks dev_err (and host_err, when given: a word of pinned host memory that receives 1 at a time-out, readable
 * by the host without touching the device; and dev_void, when given: a device word that receives 1, for consumers of the forward's
 * results on the device -- pam_set_input_guard; NULL = none).  Counters are zeroed by the caller in front of the first signal.  Flagged forwards of one process must not be in flight at the same time (their gates can block each other's queues). */
int pam_flag_signal(void* stream, int32_t* dev_counter);
/* the same add on every counter dev_counters[k] whose bit k of mask is set (k < 32), one launch, one release */
int pam_flag_signal_mask(void* stream, int32_t* dev_counters, uint32_t mask);
int pam_flag_gate(void* stream, int32_t* dev_counter, int target, int32_t* dev_err, const uint32_t* dev_max_us, int arrive, int32_t* host_err,
                  int32_t* dev_void);

/* ---- row e: the path's one exchange, in the C ABI (the reference has no distributed code -- it hands every visible GPU
 * to HRNet, /root/reference/src/ivclabpose.py:107-111,131-132).  One process per GPU; camera views are partitioned over the ranks; before
 * the cross-view match every rank contributes its views' keypoint records and receives everyone's: ONE all-gather per frame, enqueued on
 * the stream the decode ran on.  Record per view: (max_dets + 1) x 17*3 float64 -- max_dets detection rows (y, x, score), i.e. exactly
 * what pam_head_decode writes for that view when it is given max_dets + 1 as its slot stride, then one more row whose FIRST double is
 * the view's detection count; rows_per_rank = the largest number of views any rank owns (unused records are padding); dev_recv holds
 * world * rows_per_rank records, rank-major, and is what pam_frame_dev_views reads.
 * The communicator is RCCL's (ncclComm_t); librccl is bound at run time, so single-GPU hosts never need it.  pam_comm_unique_id on one
 * rank -> ship the 128 bytes to the others by any means -> pam_comm_init on every rank (collective). */
int pam_comm_unique_id(void* id128);
int pam_comm_init(void** comm, int world, int rank, const void* id128, int device);
int pam_comm_destroy(void* comm);
const char* pam_comm_last_error(void);
int pam_allgather_keypoints(PamHandle* h, void* comm, void* stream, const double* dev_send, int rows_per_rank, double* dev_recv);

/* ---- person detector side (ivclabpose.py:116-120 constructs backend.YOLOv3, :183-204 PersonDetect calls it).
 * The backend is absent from the reference tree; these follow the public Darknet YOLOv3 definition (parity unpinned).
 * pam_resize_frames: n BGR uint8 frames (dev array of dev pointers, H x W x 3) -> bilinear (cv2.resize INTER_LINEAR
 * semantics) out_h x out_w, BGR->RGB, /255, bf16 NHWC with 8 channels (RGB + 5 zeros).
 * pam_upsample_concat_nhwc_bf16: Darknet `upsample` + `route`: out[n,y,x] = concat(a[n,y/2,x/2,:Ca], b[n,y,x,:Cb]).
 * pam_yolo_detect: the three `yolo` heads (NHWC bf16, anchor-major channels [tx,ty,tw,th,obj,cls...] x 3, channel
 * stride chan_stride[h] >= 3*(5+num_classes)) -> per image the boxes of class `class_id` with
 * sigmoid(obj)*sigmoid(cls) > score_thresh, greedy NMS (IoU > nms_thresh suppressed, best score first, ties to the
 * lower candidate number: head, then cell row-major, then anchor), at most max_det rows (x1, y1, x2, y2, score) in
 * frame pixels (float32) into dev_out[n_img][max_det][5]; dev_count[i] = rows kept, dev_count[n_img + i] = boxes above
 * the threshold before NMS (only the first PAM_YOLO_MAX_CAND of them, in candidate order, enter NMS).
 * anchors: [head][anchor][w, h] in network-input pixels (18 floats, host memory). */
int pam_resize_frames(void* stream, int n, const void* const* dev_frames, int frame_h, int frame_w,
                      int out_h, int out_w, void* dev_out_bf16);
int pam_upsample_concat_nhwc_bf16(void* stream, const void* a, const void* b, void* out, int N, int H, int W, int Ca, int Cb);
int pam_yolo_detect(void* stream, int n_img, const void* const* heads /*host array of 3 dev ptrs*/, const int32_t* grid_h,
                    const int32_t* grid_w, const int32_t* chan_stride, const float* anchors, int net_w, int net_h,
                    int num_classes, int class_id, float score_thresh, float nms_thresh, int frame_w, int frame_h,
                    int max_det, float* dev_out, int32_t* dev_count);
/* pam_yolo_detect_ws (round 5): the same result with the scoring pass spread over several workgroups per image (2 048 candidates each;
 * the workgroup that finishes an image last concatenates their kept boxes in candidate order and runs the NMS).  dev_workspace: at least
 * pam_yolo_detect_workspace_bytes(n_img, grid_h, grid_w) bytes of device memory, 16-byte aligned, whose first 4 * n_img bytes are ZERO
 * before the first call (the kernel leaves them zero); one workspace serves one call at a time. */
long long pam_yolo_detect_workspace_bytes(int n_img, const int32_t* grid_h, const int32_t* grid_w);
int pam_yolo_detect_ws(void* stream, int n_img, const void* const* heads, const int32_t* grid_h, const int32_t* grid_w,
                       const int32_t* chan_stride, const float* anchors, int net_w, int net_h, int num_classes, int class_id,
                       float score_thresh, float nms_thresh, int frame_w, int frame_h, int max_det, float* dev_out, int32_t* dev_count,
                       void* dev_workspace, long long workspace_bytes);

/* One to three `yolo` heads (YOLOv3-tiny has two): the three entry points above with the number of heads stated.  heads, grid_h, grid_w
 * and chan_stride hold n_heads entries in cfg order (coarsest first); anchors: [head][anchor][w, h], 6 * n_heads floats.  Candidate order
 * is unchanged: head, then cell row-major, then anchor.  n_heads outside 1 .. 3: PAM_E_ARG (-1 from the workspace query).  The three-head
 * entry points are these with n_heads = 3. */
long long pam_yolo_detect_heads_workspace_bytes(int n_img, int n_heads, const int32_t* grid_h, const int32_t* grid_w);
int pam_yolo_detect_heads(void* stream, int n_img, int n_heads, const void* const* heads, const int32_t* grid_h, const int32_t* grid_w,
                          const int32_t* chan_stride, const float* anchors, int net_w, int net_h, int num_classes, int class_id,
                          float score_thresh, float nms_thresh, int frame_w, int frame_h, int max_det, float* dev_out, int32_t* dev_count);
int pam_yolo_detect_heads_ws(void* stream, int n_img, int n_heads, const void* const* heads, const int32_t* grid_h, const int32_t* grid_w,
                             const int32_t* chan_stride, const float* anchors, int net_w, int net_h, int num_classes, int class_id,
                             float score_thresh, float nms_thresh, int frame_w, int frame_h, int max_det, float* dev_out, int32_t* dev_count,
                             void* dev_workspace, long long workspace_bytes);
/* Darknet `maxpool` on NHWC bf16 (YOLOv3-tiny): pad = size - 1, Ho = (H - 1) / stride + 1, Wo alike; the window of output (oy, ox) starts
 * at (oy * stride - pad / 2, ox * stride - pad / 2) and taps outside the image do not take part.  out: N x Ho x Wo x C.  The result is
 * one of the inputs (bit-exact against torch.max_pool2d on the -inf-padded tensor), so zero channels stay zero.
 * C % 8 == 0, size 2 or 3, stride 1 or 2; PAM_E_ARG otherwise (null pointer included), PAM_E_HIP on a launch error. */
int pam_maxpool_nhwc_bf16(void* stream, const void* in, void* out, int N, int H, int W, int C, int size, int stride);
/* YOLOv3-SPP's block in one launch: three stride-1 Darknet `maxpool`s of one layer and the `route` over them and their source.
 * in: NHWC bf16 (N, H, W, C).  out: NHWC bf16 (N, H, W, 4C) = [pool_s3 | pool_s2 | pool_s1 | in] along the channels.  Every pool is the
 * stride-1 `maxpool` above: the window is centred on the pixel, taps outside the image do not take part.  The copy of `in` is bitwise.  A
 * pooled value is one of the window's inputs, bit for bit, wherever it is not zero; where it is zero either sign of zero may come out (the
 * sign depends on the scan order, which the kernel chooses).  NaN inputs are outside the contract.
 * PAM_E_ARG, before anything is launched, for: a null pointer; N, H or W <= 0; C % 8 != 0 (C <= 0 included); H or W above PAM_SPP_MAX_HW
 * (the largest map the kernel holds in LDS: network inputs up to 1024 x 1024); sizes that are not odd, not in 3 .. 13 or not strictly
 * ascending (s1 < s2 < s3).  PAM_E_HIP on a launch error.
 * The _slab form states the channels per workgroup (8, 16, 32 or 64, PAM_E_ARG otherwise; halved until the map fits the workgroup's LDS):
 * a measuring hook, the plain form uses the slab that measured fastest. */
#define PAM_SPP_MAX_HW 32
int pam_spp_concat_nhwc_bf16(void* stream, const void* in, void* out, int N, int H, int W, int C, int s1, int s2, int s3);
int pam_spp_concat_slab_nhwc_bf16(void* stream, const void* in, void* out, int N, int H, int W, int C, int s1, int s2, int s3, int slab);

/* ---- YOLOv4 / YOLOv4-tiny (csrc/pam_route.hip, csrc/pam_detect.hip; the public Darknet definitions of Bochkovskiy et al. 2020, parity
 * unpinned like YOLOv3's).
 * pam_route_concat_nhwc_bf16 (k_route): Darknet's general `route`, one launch.  out: NHWC bf16 (N, H, W, C_out).  Source k (n_src of
 * them, 1 .. PAM_ROUTE_MAX_SRC; src and the four tables are host arrays) is an NHWC bf16 map whose pixels are src_cstride[k] channels
 * apart; its slice is the src_count[k] channels from channel src_offset[k] (a `groups=` / `group_id=` route, or the real channels of a
 * channel-padded layer).  src_up2[k] != 0: the source is the (N, H/2, W/2) map, read at (y/2, x/2) (`upsample stride=2` in front of the
 * route); else it is (N, H, W).  out[n, y, x, :] = the slices side by side in source order, compact, then +0 (all bits zero) up to C_out.
 * A pure copy: every output bit is a source bit or zero.
 * PAM_E_ARG, before anything is launched, for: a NULL pointer (table, source or out) or one that is not 16-byte aligned; n_src outside
 * 1 .. PAM_ROUTE_MAX_SRC; N, H, W or C_out <= 0; C_out % 8 != 0; a stride, offset or count that is not a multiple of 8, a count <= 0, a
 * negative offset, or offset + count > stride (the slice leaves its source); odd H or W with an x2 source; C_out smaller than the sum of
 * the counts; N * H * W * C_out / 8 >= 2^31 (the kernel's piece index is 32-bit).  PAM_E_HIP on a launch error. */
#define PAM_ROUTE_MAX_SRC 4
int pam_route_concat_nhwc_bf16(void* stream, int n_src, const void* const* src, const int32_t* src_cstride, const int32_t* src_offset,
                               const int32_t* src_count, const int32_t* src_up2, void* out, int N, int H, int W, int C_out);
/* pam_yolo_detect_heads / _ws with YOLOv4's `scale_x_y`: scale_xy (host memory) holds one s per head, and a box centre is
 * (sigmoid(t) * s - 0.5f * (s - 1) + cell) / grid in float32, evaluated in that order.  Everything else -- candidate order (head in the
 * order given, which need not be coarsest first; then cell row-major; then anchor), scores, NMS, outputs, workspace
 * (pam_yolo_detect_heads_workspace_bytes) -- is pam_yolo_detect_heads'.  With every s = 1 the bytes are those of pam_yolo_detect_heads
 * (v * 1.0f - 0.0f is exact), which is implemented as this call with a table of ones.  PAM_E_ARG additionally for a NULL table or an s
 * that is NaN, infinite or < 1. */
int pam_yolo_detect_heads_sxy(void* stream, int n_img, int n_heads, const void* const* heads, const int32_t* grid_h, const int32_t* grid_w,
                              const int32_t* chan_stride, const float* anchors, const float* scale_xy, int net_w, int net_h, int num_classes,
                              int class_id, float score_thresh, float nms_thresh, int frame_w, int frame_h, int max_det, float* dev_out,
                              int32_t* dev_count);
int pam_yolo_detect_heads_sxy_ws(void* stream, int n_img, int n_heads, const void* const* heads, const int32_t* grid_h, const int32_t* grid_w,
                                 const int32_t* chan_stride, const float* anchors, const float* scale_xy, int net_w, int net_h,
                                 int num_classes, int class_id, float score_thresh, float nms_thresh, int frame_w, int frame_h, int max_det,
                                 float* dev_out, int32_t* dev_count, void* dev_workspace, long long workspace_bytes);

/* ---- baseline JPEG frames decoded on the device behind a host entropy pass (csrc/pam_jpeg_entropy.hpp, csrc/pam_jpeg.hip; the
 * reference decodes with one cv2.imread per camera per frame on the main thread, dataset.py:36-45).  The host does the serial half --
 * header parse and Huffman decode into quantised coefficients -- and the device the parallel half: dequantisation, inverse DCT, chroma
 * upsampling, colour conversion and the store as BGR uint8 (H, W, 3), cv2.imread's layout.  The bytes are those of libjpeg's default
 * decode (slow-integer DCT, fancy upsampling), i.e. of PIL.Image.open(..).convert('RGB') with the channels flipped.
 *
 * Files taken: SOF0 (baseline), 8-bit samples, Huffman coding, ONE interleaved scan, 8-bit quantisation tables; one component, or three
 * YCbCr components with chroma 1x1 and luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0); byte stuffing, FF fill bytes in front of markers,
 * restart intervals (DRI, RST0-7); APPn / COM skipped, bytes behind the scan's end ignored.  Everything else is reported in
 * PamJpegInfo.unsupported and left to another decoder; it is not an error. */
#define PAM_JPEG_U_NOT_JPEG 1    /* no SOI */
#define PAM_JPEG_U_PROGRESSIVE 2 /* SOF2 */
#define PAM_JPEG_U_ARITHMETIC 3  /* SOF9-11, 13-15, DAC */
#define PAM_JPEG_U_SOF 4         /* SOF1 (extended sequential), lossless and differential frames */
#define PAM_JPEG_U_PRECISION 5   /* samples of other than 8 bits */
#define PAM_JPEG_U_QUANT16 6     /* a 16-bit quantisation table */
#define PAM_JPEG_U_COMPONENTS 7  /* neither one nor three components (CMYK / YCCK) */
#define PAM_JPEG_U_COLORSPACE 8  /* three components that are not YCbCr: Adobe APP14 with a transform other than 1, or ids R, G, B without JFIF */
#define PAM_JPEG_U_SAMPLING 9    /* sampling factors other than the three above (4:4:0, 4:1:1, subsampled luma, ...) */
#define PAM_JPEG_U_SCAN 10       /* the first scan does not hold all components in frame order with Ss = 0, Se = 63, Ah = Al = 0 */
#define PAM_JPEG_U_DNL 11        /* zero height / a DNL marker */

/* What the header of a file says, and where the entropy pass puts its coefficients.  Component c's blocks start at word coef_offset[c]
 * of the coefficient buffer: blocks_h[c] rows of blocks_w[c] blocks, row-major, 64 int16 each in natural (row-major, de-zigzagged)
 * order, QUANTISED (as coded; the device multiplies by quant[c]).  blocks_w[c] = mcu_w * h_samp[c], blocks_h[c] = mcu_h * v_samp[c]:
 * the padding blocks of partial MCUs are included.  coef_words = 64 * all blocks; the component planes the device writes take
 * coef_words BYTES (one uint8 per coefficient; component c's plane at byte coef_offset[c], blocks_w[c] * 8 bytes per row). */
typedef struct PamJpegInfo {
    int32_t width, height, n_comp;
    int32_t unsupported;         /* 0 = taken, else PAM_JPEG_U_*: the fields behind what the parser had read by then are zero */
    int32_t h_samp[3], v_samp[3];
    int32_t mcu_w, mcu_h;        /* MCUs per row, MCU rows */
    int32_t blocks_w[3], blocks_h[3];
    int32_t restart_interval;    /* MCUs between RSTn markers, 0 = none */
    int32_t reserved;
    int64_t coef_offset[3];      /* int16 words */
    int64_t coef_words;
    uint16_t quant[3][64];       /* per component, natural order */
} PamJpegInfo;

/* pam_jpeg_probe: SOI through SOS of the n bytes at data -> *info.  PAM_OK with info->unsupported = 0 or a reason; PAM_E_ARG for a
 * header that is cut short or corrupt (*info is then not to be used).
 * pam_jpeg_entropy: the scan of a file the probe took -> coef[0 .. info->coef_words), zeros where nothing is coded.  PAM_E_ARG when
 * coef_words < info->coef_words, when *info does not belong to the file, and for a stream that is cut short or corrupt (an undefined
 * code, a run that leaves its block, a missing or wrong restart marker): what decoded until then is in coef.
 * Neither has a handle, global state or a HIP call: any number of threads may run them at once.  Neither reads outside data[0 .. n) or
 * writes outside coef[0 .. coef_words), whatever the bytes are. */
int pam_jpeg_probe(const uint8_t* data, size_t n, PamJpegInfo* info);
int pam_jpeg_entropy(const uint8_t* data, size_t n, const PamJpegInfo* info, int16_t* coef, size_t coef_words);

/* One image of a reconstruction.  dev_coef: info.coef_words int16 as the entropy pass wrote them; dev_quant: n_comp * 64 uint16
 * (info.quant); dev_planes: info.coef_words bytes of scratch (written in full, never read before written); dev_out: height * width * 3
 * bytes, B, G, R per pixel.  dev_coef, dev_quant and dev_planes are 16-byte aligned, dev_out 4-byte aligned.  h_samp, v_samp: the luma
 * sampling factors (1, 1 for one component); the block counts follow from these five integers as PamJpegInfo states them. */
typedef struct PamJpegImage {
    const int16_t* dev_coef;
    const uint16_t* dev_quant;
    uint8_t* dev_planes;
    uint8_t* dev_out;
    int32_t width, height, n_comp, h_samp, v_samp, reserved;
} PamJpegImage;

/* pam_jpeg_reconstruct: n_img (1 .. PAM_MAX_VIEWS) images of any mix of sizes and samplings in ONE launch pair on `stream`; images is a
 * host array, copied into the kernel arguments.  Every byte of every dev_out is written, nothing outside it.  PAM_E_ARG, before anything
 * is launched, for a null or misaligned pointer, a size outside 1 .. 65535, and a component count or sampling outside the list above.
 *
 * k_jpeg_idct, per 8x8 block: v = coef * quant, then one 1-D pass down the columns with s = 11 and one along the rows with s = 18, then
 * + 128, clamped to 0 .. 255.  All int32 (wrapping), >> arithmetic.  The 1-D pass on x0 .. x7:
 *   z1 = (x2 + x6) * 4433;  t2 = z1 - x6 * 15137;  t3 = z1 + x2 * 6270;  t0 = (x0 + x4) << 13;  t1 = (x0 - x4) << 13
 *   t10 = t0 + t3;  t13 = t0 - t3;  t11 = t1 + t2;  t12 = t1 - t2;  a0 = x7;  a1 = x5;  a2 = x3;  a3 = x1
 *   z1 = a0 + a3;  z2 = a1 + a2;  z3 = a0 + a2;  z4 = a1 + a3;  z5 = (z3 + z4) * 9633
 *   a0 *= 2446;  a1 *= 16819;  a2 *= 25172;  a3 *= 12299;  z1 *= -7373;  z2 *= -20995;  z3 = z3 * -16069 + z5;  z4 = z4 * -3196 + z5
 *   a0 += z1 + z3;  a1 += z2 + z4;  a2 += z2 + z3;  a3 += z1 + z4
 *   out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], each (v + (1 << (s - 1))) >> s
 * k_jpeg_color, per output pixel, with w = ceil(W / 2), h = ceil(H / 2) the TRUE subsampled extents and neighbours clamped to them:
 *   2x1:  out[2i] = (3 p[i] + p[i-1] + 1) >> 2,  out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2
 *   2x2:  s[i] = 3 p[r][i] + p[r'][i], r' the row above (even output row) or below (odd);  out[2i] = (3 s[i] + s[i-1] + 8) >> 4,
 *         out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4
 *   cb -= 128, cr -= 128;  R = Y + ((91881 cr + 32768) >> 16);  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16);
 *   B = Y + ((116130 cb + 32768) >> 16), clamped to 0 .. 255; one component: B = G = R = Y. */
int pam_jpeg_reconstruct(void* stream, int n_img, const PamJpegImage* images);

/* ---- baseline JPEG frames ENCODED behind the device (csrc/pam_jpeg_fwd.hip, csrc/pam_jpeg_encode.hpp; the reference saves its annotated
 * frames with one cv2.imwrite per camera per frame on the main thread, testmodel.py:76-80).  The mirror image of the decode: the device does
 * the parallel half -- colour conversion, chroma downsampling, forward DCT, quantisation -- into the coefficient layout PamJpegInfo
 * describes, and the host the serial half, the Huffman pass and the file's headers.  The arithmetic is libjpeg's default encoder (slow-
 * integer DCT, standard Huffman tables, JFIF header), so at quality 75 and 4:2:0 the file is byte for byte what
 * PIL.Image.fromarray(rgb).save(path) writes from the same pixels.  Three components; luma sampling 1x1, 2x1 or 2x2, chroma 1x1. */

/* One image of a forward pass.  dev_bgr: height * width * 3 bytes, B, G, R per pixel, any alignment; dev_quant: 3 * 64 uint16, per
 * component in natural order (pam_jpeg_quality_tables writes them); dev_coef: the int16 buffer of PamJpegInfo's layout for these five
 * integers (64 * (mw hs mh vs + 2 mw mh) words with mw = ceil(width / (8 hs)), mh = ceil(height / (8 vs))), written IN FULL: the padding
 * blocks of partial MCUs as zeros, so the buffer can go to pam_jpeg_reconstruct as it is.  dev_quant and dev_coef are 16-byte aligned. */
typedef struct PamJpegFwdImage {
    const uint8_t* dev_bgr;
    const uint16_t* dev_quant;
    int16_t* dev_coef;
    int32_t width, height, h_samp, v_samp;
} PamJpegFwdImage;

/* pam_jpeg_forward: n_img (1 .. PAM_MAX_VIEWS) images of any mix of sizes and samplings in ONE launch on `stream`; images is a host array,
 * copied into the kernel arguments.  PAM_E_ARG, before anything is launched, for a null or misaligned pointer, a size outside 1 .. 65535,
 * a sampling outside the three above.  The quantisation tables are device memory and not looked at: the kernel takes a zero as 1.
 *
 * Per component c (h_c, v_c its sampling, h_max x v_max the luma's): wb = ceil(ceil(W h_c / h_max) / 8) real blocks per row, hb likewise;
 * the other blocks of the layout are zeros.  Samples of a real block, all int32, >> arithmetic:
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   not subsampled: sample (y, x) is pixel (min(y, H - 1), min(x, W - 1)).
 *   subsampled chroma: sample (y, x) with y' = min(y, ceil(H / v_max) - 1) averages the pixels (min(v_max y' + dy, H - 1),
 *   min(h_max x + dx, W - 1)):  2x2: (p00 + p01 + p10 + p11 + bias) >> 2, bias 1 for even x, 2 for odd;  2x1: (p0 + p1 + bias) >> 1,
 *   bias 0 for even x, 1 for odd.
 * Forward DCT on sample - 128, along the rows first, then down the columns, with the constants of the inverse pass above.  On d0 .. d7:
 *   t0..t3 = d0+d7, d1+d6, d2+d5, d3+d4;  t7..t4 = d0-d7, d1-d6, d2-d5, d3-d4;  t10 = t0+t3; t13 = t0-t3; t11 = t1+t2; t12 = t1-t2
 *   rows: o0 = (t10+t11) << 2, o4 = (t10-t11) << 2;  columns: o0 = (t10+t11+2) >> 2, o4 = (t10-t11+2) >> 2
 *   z1 = (t12+t13) * 4433;  o2 = z1 + t13 * 6270;  o6 = z1 - t12 * 15137
 *   z1 = t4+t7; z2 = t5+t6; z3 = t4+t6; z4 = t5+t7; z5 = (z3+z4) * 9633
 *   t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
 *   o7 = t4+z1+z3; o5 = t5+z2+z4; o3 = t6+z2+z3; o1 = t7+z1+z4;  o1, o2, o3, o5, o6, o7: (v + (1 << (s - 1))) >> s, s = 11 rows, 15 columns
 * Quantisation of c with qv = 8 quant: sign(c) * ((|c| + (qv >> 1)) / qv), the division truncating. */
int pam_jpeg_forward(void* stream, int n_img, const PamJpegFwdImage* images);

/* What the entropy encoder needs besides the coefficients.  quality 1 .. 100: the tables of pam_jpeg_quality_tables (quant is ignored);
 * quality 0: quant[0] for the luma and quant[1] for both chroma components, natural order, every entry 1 .. 255. */
typedef struct PamJpegEncodeParams {
    int32_t width, height, h_samp, v_samp;
    int32_t quality, reserved;
    uint16_t quant[2][64];
} PamJpegEncodeParams;

/* pam_jpeg_quality_tables: libjpeg's tables for a quality of 1 .. 100 -> tables[0] (luma), tables[1] (chroma), natural order: the tables
 * of Annex K of the standard, each entry (base * scale + 50) / 100 clamped to 1 .. 255 with scale = 5000 / quality below 50, else
 * 200 - 2 quality.  PAM_E_ARG: a null pointer, a quality outside 1 .. 100.
 * pam_jpeg_encode_bound: *bytes = a capacity that pam_jpeg_encode never exceeds for an image of this size and sampling, whatever the
 * coefficients: 625 header and trailer bytes + 420 for every coded block.  PAM_E_ARG: a null pointer, a size outside 1 .. 65535, a
 * sampling outside the three above.
 * pam_jpeg_encode: coef[0 .. coef_words) in PamJpegInfo's layout (as pam_jpeg_forward or pam_jpeg_entropy wrote them) -> a complete file
 * in out[0 .. *out_bytes), *out_bytes <= capacity.  SOI; APP0 (JFIF 1.01, no units, density 1 x 1, no thumbnail); two DQT segments in
 * zigzag order; SOF0 (ids 1, 2, 3; luma h << 4 | v, chroma 0x11; tables 0, 1, 1); four DHT segments DC0, AC0, DC1, AC1 with the tables of
 * Annex K.3 - K.6; SOS; one MCU-interleaved scan (DC difference category + value bits, AC run/size with ZRL and EOB, FF stuffed with 00,
 * the last byte padded with one-bits); EOI.  The padding blocks of partial MCUs are NOT read: each is coded as all-zero AC with the DC of
 * the block coded just before it.
 * PAM_E_ARG, with out[capacity ..) untouched whatever was written below it: a null pointer, what pam_jpeg_encode_bound refuses,
 * coef_words below the layout's, a quality outside 0 .. 100 or a table entry outside 1 .. 255 at quality 0, a capacity the file does not
 * fit in, and a coefficient the standard tables have no code for (a DC difference beyond 11 bits, an AC value beyond 10).
 * None of the three has a handle, global state, an allocation or a HIP call: any number of threads may run them at once. */
int pam_jpeg_quality_tables(int quality, uint16_t* tables);
int pam_jpeg_encode_bound(int width, int height, int h_samp, int v_samp, size_t* bytes);
int pam_jpeg_encode(const int16_t* coef, size_t coef_words, const PamJpegEncodeParams* params, uint8_t* out, size_t capacity, size_t* out_bytes);

/* ---- the overlay of the tracked skeletons drawn on the device (csrc/pam_overlay.hip; the host form is visualization.
 * draw_points_and_skeleton, which the reference's demo loop calls once per person and view, testmodel.py:70-75).  This is the project's
 * own rasteriser, defined in integers so that it can be restated exactly (tests/overlay_ref.py); it is not PIL's.
 *
 * A primitive is a capsule: every pixel within hw of the segment A - B, in units of 1/8 pixel (the host quantises a coordinate v to
 * floor(8 v + 0.5) and drops what is not finite or beyond 2^18 in magnitude).  A joint's disc is the capsule with A = B and hw = 8 r.
 * Pixel (px, py) has its centre at P = (8 px, 8 py).  With d = B - A, p = P - A, t = p . d, all int64:
 *   t <= 0:      inside iff |p|^2 <= hw^2
 *   t >= d . d:  inside iff |P - B|^2 <= hw^2
 *   else:        inside iff |cross(p, d)| < 2^31 and cross^2 <= hw^2 (d . d)
 * Of all primitives of its view that cover a pixel, the LAST in table order gives the pixel its colour; a pixel none covers is not
 * written. */
typedef struct PamOverlayPrim {
    int32_t ax, ay, bx, by;      /* 1/8 pixel, |.| <= 2^18 */
    int32_t hw;                  /* 1/8 pixel, 0 .. 2^12 */
    uint32_t bgr;                /* B | G << 8 | R << 16 */
    int32_t reserved[2];
} PamOverlayPrim;

/* One view of a draw: its frame, BGR uint8 (height, width, 3), drawn in place, and its primitives prim_first .. prim_first + prim_count
 * of the table, in painter's order. */
typedef struct PamOverlayView {
    uint8_t* dev_bgr;
    int32_t width, height;
    int32_t prim_first, prim_count;
} PamOverlayView;

/* pam_overlay_draw: n_views (1 .. PAM_MAX_VIEWS) views of any mix of sizes in ONE launch on `stream`; views is a host array, copied
 * into the kernel arguments; dev_prims: n_prims primitives in device memory, 16-byte aligned (may be null when n_prims is 0: nothing is
 * launched).  One workgroup per 64 x 16 pixel tile: it culls its view's primitives against the tile by their bounding boxes into LDS
 * and leaves when none is left.  A primitive whose coordinates or hw are outside the ranges above is not drawn.  PAM_E_ARG, before
 * anything is launched: a null views or frame pointer, n_views outside 1 .. 32, a size outside 1 .. 65535, a range of primitives that
 * leaves the table. */
int pam_overlay_draw(void* stream, int n_views, const PamOverlayView* views, const PamOverlayPrim* dev_prims, int n_prims);

/* pam_overlay_draw_counted: pam_overlay_draw with the views' primitive counts read on the device (the same kernel with one more
 * pointer): view i draws the first clamp(dev_count[i], 0, views[i].prim_count) primitives of its range, so a device count never reaches
 * past the range the host names.  Workgroups are launched for every view whose host-side prim_count is positive; a tile of a view
 * whose device count is 0 leaves at once.  For the fixed-layout table of pam_overlay_tracks, whose ranges are mostly null rows that
 * every tile would otherwise cull.  PAM_E_ARG: what pam_overlay_draw refuses, and a null dev_count (n_views int32 in device memory). */
int pam_overlay_draw_counted(void* stream, int n_views, const PamOverlayView* views, const PamOverlayPrim* dev_prims, int n_prims,
                             const int32_t* dev_count);

/* ---- the overlay's primitive table from the tracker state (csrc/pam_overlay_tracks.hip; the host form is visualization.track_rows +
 * overlay_table on a fetched record) and the free-viewpoint 3D view (the plot3DPose the reference's demo loop calls and does not ship,
 * testmodel.py:77-81: "you can design your own method to visualize 3D poses") -----------------------------------------------------------
 * pam_overlay_tracks (k_overlay_tracks: one workgroup, asynchronous on `stream`) reads the state of `scene` as the frame launches already
 * on `stream` leave it, writes nothing to it and does not look at the input guard.  The host never learns a count.
 *   tracks      in list order (the record's order), positions 0 .. n_tracks - 1; with emitted_only != 0 only the tracks the record calls
 *               emitted: time_since_update == 0 and Confirmed (ivclabpose.py:266).
 *   pose        of the track at list position i: row i of dev_pose (17 x 3 doubles; pam_one_euro's dev_pose of this scene) when that
 *               pointer is given, else the newest pose of the track's history ring -- the record's pose3d.
 *   view v      views[v].camera = c in 0 .. C - 1: P = the handle's camera c (pam_set_cameras; float32); camera = -1: P = row
 *               views[v].extra of dev_extra_P (12 float32 each, row-major 3 x 4; device memory).
 *   projection  of joint (X, Y, Z), P promoted to double, sums left to right:
 *                 h0 = P[0] X + P[1] Y + P[2] Z + P[3];  h1 = P[4] X + ... + P[7];  h2 = P[8] X + ... + P[11]
 *                 ih = 1.0 / h2;  u = h0 * ih (column);  w = h1 * ih (row)
 *               While a lens table is set (pam_set_lens) and the row of camera c has a non-zero coefficient, (u, w) then goes through
 *               normalise, forward and pixels of the lens section above, as in pam_track_boxes: the skeleton lies on the RAW image.  Extra
 *               views have no lens.  The library is built with -ffp-contract=off: computed as written, the division is the device's.
 *   drawable    a joint: h2 > 0.0, u and w finite, and qx = floor(8.0 * u + 0.5), qy = floor(8.0 * w + 0.5) both within 2^18 in
 *               magnitude.  A limb: both of its joints.
 *   rows        of view v in painter's order: per track the 19 COCO limbs (a, b) in the order (15,13) (13,11) (16,14) (14,12) (11,12)
 *               (5,11) (6,12) (5,6) (5,7) (6,8) (7,9) (8,10) (1,2) (0,1) (0,2) (1,3) (2,4) (0,5) (0,6), then the 17 joints.
 *               limb:  A = (qx, qy) of a, B = that of b, hw = 4 * limb_width, bgr = palette[track id mod 8] (the non-negative remainder)
 *               joint: A = B = (qx, qy), hw = 8 * radius, bgr = palette[8 + j];  reserved words 0
 *               radius = max(2, the integer nearest min(width, height) / 150.0, ties to even), limb_width = radius / 2 + 1 (integer
 *               division), from the view's width and height: the frame it will be drawn into.
 *   layout      view v owns rows [v * cap, (v + 1) * cap) of dev_prims.  Its drawable rows stand at the front in the order above,
 *               dev_count[v] is their number, and every other row of the range is a null row (hw = -1, all else 0: pam_overlay_draw*
 *               skips it).  All n_views * cap rows are defined after the launch and nothing outside them is written.
 * For a pin-hole camera this is the table visualization.overlay_table(track_rows(...)) builds from the fetched record (to the ulp by
 * which the one-division projection may differ from h0 / h2).
 * palette: 25 host words B | G << 8 | R << 16, copied into the launch: 8 limb colours, then the 17 joint colours.
 * PAM_E_ARG, before any device call: a NULL handle, views, palette, dev_prims or dev_count; n_views outside 1 .. PAM_MAX_VIEWS; a camera
 * outside -1 .. C - 1; an extra row outside 0 .. n_extra - 1 (n_extra > 0 needs dev_extra_P); a width or height outside 1 .. 65535;
 * cap < PAM_OVERLAY_TRACK_ROWS * max_tracks (or > 2^20); dev_prims not 16-byte aligned; a scene the handle does not have.
 * PAM_E_STATE: pam_set_cameras has not been called. */
#define PAM_OVERLAY_TRACK_ROWS 36    /* rows of one track in one view: 19 limbs + 17 joints */
typedef struct PamOverlayTrackView {
    int32_t camera;              /* 0 .. C - 1: a camera of the handle; -1: extra view `extra` */
    int32_t extra;               /* row of dev_extra_P when camera == -1 */
    int32_t width, height;       /* of the frame the view is drawn into: fixes joint radius and limb width */
} PamOverlayTrackView;
int pam_overlay_tracks(PamHandle* h, void* stream, int scene, int n_views, const PamOverlayTrackView* views, const float* dev_extra_P,
                       int n_extra, const double* dev_pose, const uint32_t* palette, int emitted_only, int cap,
                       PamOverlayPrim* dev_prims, int32_t* dev_count);

#ifdef __cplusplus
}
#endif
#endif /* PAM_H */
