/* libwatsor_hip.so -- C ABI of the MI355X detection backend for Watsor.
 *
 * The reference has no FFI on this path: the boundary is a duck-typed Python plugin
 * (`watsor/detection/tensorflow_cpu.py:13,64-92`, `watsor/detection/tensorrt_gpu.py:20,55-91`)
 * driven by `ObjectDetector._next_frame` (`watsor/detection/detector.py:102-112`).  This header is
 * what sits *behind* the Python class `watsor_amd.detection.hip_gpu.HipObjectDetector`: plain
 * pointers and sizes, no torch / numpy types.  Every entry point names the reference code it
 * stands in for.  INTEGRATION.md shows the ctypes binding and the two-line change in
 * `watsor/detection/detector.py` that enables it.
 *
 * Conventions: all functions return 0 on success or a negative WZ_E* code; `wz_last_error()`
 * returns a human readable message for the calling thread's last failure.  One engine = one GPU
 * with up to WZ_SLOTS lanes (a lane = one in-flight batch: its own HIP stream, activation buffers
 * and captured graph; wz_num_slots() tells how many, 4 unless WZ_LANES says otherwise); calls on
 * one engine must be serialised by the caller (the reference worker is sequential per detector
 * instance, detector.py:84-112) -- the lanes overlap on the GPU, not on the host.  Host frames are packed RGB24, HWC,
 * C-contiguous (`Frame.get_numpy_image`, watsor/stream/share.py:68-73); they are read only and
 * not retained past the call.
 *
 * Environment (read when the first engine of a process is created): WZ_LANES=1..8 (batches in flight, default 4), WZ_STREAMS (HIP
 * streams they ride, default = lanes, at most 4 pay), WZ_GRAPH=0|1 (launch kernel by kernel / replay a captured graph; unset: under the throughput schedule a captured graph while another lane is busy and
 * kernel by kernel for a batch that finds the other lanes idle, under the latency schedule always kernel by kernel),
 * WZ_SCHEDULE=latency (launch shapes for the shortest lone batch instead of the most frames per second with every lane busy).
 * GPU_MAX_HW_QUEUES (the HIP runtime's: hardware queues of this process) is WRITTEN when the library loads: four lanes need a queue each
 * beside the runtime's own, so a value that is unset, empty, not a number or below 8 becomes 8; 8 and more is left as the host set it
 * (wz_hw_queues()).  It takes effect only where the library is loaded before the process's first HIP call.
 */
#ifndef WATSOR_HIP_H
#define WATSOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WZ_MAX_DETECTIONS 100 /* Header.detections length, watsor/stream/share.py:31 */
#define WZ_MAX_ZONES 10       /* Detection.zones length,   watsor/stream/share.py:22 */
#define WZ_NUM_LABELS 91      /* len(COCO_CLASSES),        watsor/config/coco.py:14-106 */
#define WZ_MAX_CAMS 256       /* camera ids with a GPU filter (wz_set_camera_filter) per engine: 0 .. WZ_MAX_CAMS - 1 */

#define WZ_OK 0
#define WZ_EINVAL (-1)   /* bad argument */
#define WZ_ENOENT (-2)   /* engine file missing  -> Python raises FileNotFoundError (detector.py:97-98) */
#define WZ_EFORMAT (-3)  /* engine file corrupt / wrong version */
#define WZ_EHIP (-4)     /* HIP runtime error (message has the hipError string) */
#define WZ_ENODEV (-5)   /* no such GPU */
#define WZ_ELIMIT (-6)   /* batch / resolution / camera id beyond what wz_create() reserved */
#define WZ_EINCOMPLETE (-7) /* the call DID its work -- every row was written -- but a frame's rows may be short (clip-after-NMS engines: more
                             * selected boxes lay entirely outside the image than the walk keeps in reserve; wz_collect / wz_collect_bound /
                             * wz_detect_batch).  Every other code means the rows were NOT written.  -> Python raises RowsIncomplete */

/* Byte-for-byte `Detection` of watsor/stream/share.py:11-25 (72 bytes; label@0 zones@4
 * confidence@48 bounding_box@56).  Rows are written in place. */
typedef struct wz_detection {
    int32_t label;
    int32_t zones[WZ_MAX_ZONES];
    int32_t _pad;
    double confidence;
    int32_t x_min, y_min, x_max, y_max;
} wz_detection_t;

typedef struct wz_engine wz_engine_t;

/* ---- device enumeration: what `cuda_gpus()` does with pycuda (watsor/detection/devices.py:28-77) */
int wz_device_count(void);
int wz_device_name_of(int device, char* buf, int buflen);
/* PCI address of a device ("0000:c1:00.0"; buflen >= 16): the key of /sys/bus/pci/devices/<id>/numa_node and local_cpulist, by which
 * a detector process pins itself -- and with it the first-touch placement of the frame memory it page-locks -- to the GPU's NUMA node
 * (the reference starts one detector process per device, watsor/detection/detector.py:34-50, watsor/main.py:414-418). */
int wz_device_pci_bus_id(int device, char* buf, int buflen);
/* GPU_MAX_HW_QUEUES in this process's environment after the library loaded (0: not a number) -- what the HIP runtime reads at its
 * first call.  At least 8 unless the variable was changed afterwards; a process that initialised HIP before it loaded the library
 * runs on whatever was there then.  An engine wants 2 x wz_num_slots() (hip_gpu.py warns below that). */
int wz_hw_queues(void);

/* ---- the schedule of this process: which of two sets of launch shapes its engines use.  THROUGHPUT (default): most frames per second
 * with every lane busy.  LATENCY: the shortest lone batch -- the reference's normal load is one frame at a time per detector
 * (`_next_frame`, detector.py:102-112).  Process-wide; call before the first wz_create (the shapes are fixed when first asked for;
 * afterwards only the value already in force is accepted).  Unset: WZ_SCHEDULE in the environment decides.  Plugin option:
 * hip_options={"schedule": "latency" | "throughput" | "auto"} (watsor_amd/detection/hip_gpu.py). */
#define WZ_SCHEDULE_THROUGHPUT 0
#define WZ_SCHEDULE_LATENCY 1
int wz_set_schedule(int schedule);
int wz_get_schedule(void);

/* ---- lifecycle: TensorRTObjectDetector.__init__/__exit__ (tensorrt_gpu.py:20-53,62-63)
 * engine_path: file written by `python -m watsor_amd.engine` (the analogue of gpu.trt).
 * max_batch frames per call, each at most max_width x max_height. */
int wz_create(const char* engine_path, int device, int max_batch, int max_width, int max_height,
              wz_engine_t** out);
void wz_destroy(wz_engine_t* e);
const char* wz_device_name(wz_engine_t* e);          /* plugin property `device_name` */
const char* wz_last_error(void);

/* ---- the hot call: `detect(image_shape, image_np, detections) -> ms`
 * (tensorflow_cpu.py:74-92 / tensorrt_gpu.py:65-91) for n frames at once.
 *   rgb[i]   host pointer to frame i (h[i] x w[i] x 3 uint8)
 *   cam[i]   camera id whose filter (wz_set_camera_filter) is applied to frame i, or -1; cam may be NULL
 *   out[i]   100 Detection rows of frame i, ALL rewritten (rows past the detections carry label 1,
 *            confidence 0, box 0 exactly like the TF graph's zero padding + label offset)
 *   pass[i]  optional (may be NULL / pass may be NULL): 100 bytes, 1 where the row survives
 *            `label > 0 and Confidence and Area and Mask` (watsor/filter/track.py:26)
 *   ms[i]    wall time of the batch in milliseconds (every frame of a batch reports the batch time)
 */
int wz_detect_batch(wz_engine_t* e, int n, const uint8_t* const* rgb, const int* w, const int* h,
                    const int* cam, wz_detection_t* const* out, uint8_t* const* pass, float* ms);

/* Same, frames already resident in this GPU's HBM (device pointers).  Split into an asynchronous
 * submit (everything enqueued on the engine's stream, results land in pinned slot `slot`) and a
 * collect that waits for that slot -- so a caller can keep WZ_SLOTS batches in flight. */
#define WZ_SLOTS 8
int wz_submit_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_rgb, const int* w,
                     const int* h, const int* cam);
/* The same with HOST frame pointers (as wz_detect_batch takes them): each lane has its own staging area, the copies
 * ride the lane's stream, so the H2D of one batch overlaps the kernels of the batches on the other lanes. */
int wz_submit_host(wz_engine_t* e, int slot, int n, const uint8_t* const* rgb, const int* w,
                   const int* h, const int* cam);
/* ---- other pixel formats (the decoder side).  The reference's decoders write rawvideo RGB24 because its schema
 * says so (`watsor/config/schema.py:161`, `watsor/stream/ffmpeg.py:78-88` reads whatever the decoder writes into the
 * FrameBuffer); a decoder told `-pix_fmt nv12` / `yuv420p` writes half the bytes, and the colour conversion ffmpeg would have
 * done on the host happens in the resize kernel (8-bit, nearest chroma, 8.8 fixed point; csrc/k_preprocess.hip).  A USB / V4L2
 * camera or capture card writes packed 4:2:2 (`yuyv422` / `uyvy422`), an IR / thermal camera `gray`, an OpenCV producer `bgr24`.
 *   fmt[i]  the format word of frame i: a base format WZ_FMT_* in bits 0-7, or'ed with colour flags; fmt == NULL: all RGB24.
 *           NV12 / I420 frames are w*h*3/2 bytes and need even w and h; YUYV422 / UYVY422 are 2*w*h bytes and need even w;
 *           GRAY8 is w*h bytes, BGR24 3*w*h.  The two 10-bit 4:2:0 formats (P010, YUV420P10: what an HEVC Main10 stream decodes
 *           to) hold one little-endian 16-bit word per sample, are 3*w*h bytes -- as many as RGB24: what they save is the host's
 *           conversion, not bytes -- and need even w and h; a frame may sit at any byte address.
 *   flags   how the YUV formats (NV12, I420, YUYV422, UYVY422, P010, YUV420P10) turn into RGB.  No flag: BT.601 limited range (what the
 *           words 1 and 2 have always meant).  WZ_CSP_BT709: the BT.709 matrix (what swscale applies to a 720p / 1080p stream tagged
 *           bt709).  WZ_RANGE_FULL: Y, U, V use 0..255 (ffmpeg's yuvj* formats: MJPEG cameras).  A flag on RGB24, BGR24 or GRAY8,
 *           any other bit, and every other base format (7 to 15, 18 and above) are refused (WZ_EINVAL).
 * The three calls are the ones above with that one argument more. */
#define WZ_FMT_RGB24 0
#define WZ_FMT_NV12 1   /* h x w luma, then h/2 x w/2 interleaved (U, V) */
#define WZ_FMT_I420 2   /* h x w luma, then the h/2 x w/2 U plane, then the V plane (ffmpeg's yuv420p) */
#define WZ_FMT_YUYV422 3   /* packed Y0 U Y1 V, 2 bytes per pixel, even w (ffmpeg's yuyv422) */
#define WZ_FMT_UYVY422 4   /* packed U Y0 V Y1 (ffmpeg's uyvy422) */
#define WZ_FMT_GRAY8 5     /* one byte per pixel, R = G = B = Y, no scaling (ffmpeg's `gray` is full range) */
#define WZ_FMT_BGR24 6     /* RGB24 with the first and third byte swapped */
#define WZ_FMT_P010 0x10       /* 10-bit: h x w luma words, the sample in the HIGH bits (word >> 6; the low 6 bits are ignored), then h/2 x w/2 (U, V) word pairs (ffmpeg's p010le) */
#define WZ_FMT_YUV420P10 0x11  /* 10-bit: h x w luma words, the sample in the LOW bits (word & 0x3ff; the high 6 bits are ignored), then the U plane, then the V plane (ffmpeg's yuv420p10le) */
#define WZ_FMT_BASE_MASK 0xff
#define WZ_CSP_BT709 0x100    /* matrix; absent: BT.601 */
#define WZ_RANGE_FULL 0x200   /* Y, U, V use 0..255 (the yuvj* formats); absent: limited range */
int wz_detect_batch_fmt(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt,
                        const int* cam, wz_detection_t* const* out, uint8_t* const* pass, float* ms);
int wz_submit_device_fmt(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h,
                         const int* fmt, const int* cam);
int wz_submit_host_fmt(wz_engine_t* e, int slot, int n, const uint8_t* const* frames, const int* w, const int* h,
                       const int* fmt, const int* cam);
uint64_t wz_frame_bytes(int w, int h, int fmt);   /* bytes of one frame; 0 for a format / size the engine does not take */
/* Page-lock / release a host range that frames are handed over from (the reference's FrameBuffer arenas,
 * watsor/stream/share.py:35-41): copies out of it become DMA transfers at PCIe rate, and a frame whose height is at least twice the
 * network's input (the bilinear resize then skips rows) is not copied at all -- the resize kernel reads its tap rows IN PLACE through
 * the range's device mapping.  Either way a submitted frame must stay unchanged until its batch is collected. */
int wz_host_register(wz_engine_t* e, void* ptr, uint64_t bytes);
int wz_host_unregister(wz_engine_t* e, void* ptr);
int wz_collect(wz_engine_t* e, int slot, wz_detection_t* const* out, uint8_t* const* pass);
/* ---- tiled detection.  The network sees 300 x 300 pixels whatever the camera delivers: in a 1080p frame a person
 * 40 pixels tall arrives 11 pixels tall.  A tiled call runs the detector on rectangles of the frame instead -- a grid of overlapping tiles,
 * the whole frame as one more tile, a single region of interest -- and reports ONE list of Detection[100] rows per frame, in frame
 * coordinates.  On the lane's stream: a crop launch copies every tile into a contiguous image of the frame's own pixel format (the
 * colour flags of the format word carry over), the tiles run as an ordinary batch without cameras, and a merge launch (one workgroup per
 * frame) shifts each tile's rows by the tile's origin, thins them and applies the frame's camera filter to the 100 rows it keeps.
 *   n_tiles[i], tiles[i]   the rectangles of frame i, in pixels: 1 .. WZ_MAX_TILES of them; all the tiles of a call are one batch, so
 *                          their number may not exceed max_batch, and no tile may be larger than max_width x max_height
 *   iou_thr, ios_thr       the merge: the tiles' rows with label > 0 and confidence > 0, ordered by confidence (ties: tile, then row), are
 *                          walked in that order; a row is dropped iff a row already kept with the SAME label overlaps it by more than
 *                          iou_thr (intersection over union) or by more than ios_thr of the smaller of the two boxes (an object cut by a
 *                          tile's border against its whole box from the neighbouring or the full-frame tile).  Box sides are x_max - x_min
 *                          and y_max - y_min, in int64; a threshold >= 1 switches its test off.  100 rows are kept, zones 0; the rest are the
 *                          engine's padding rows (label 1, confidence 0, box 0); then the camera filter runs as wz_filter_rows does.
 * fmt / cam / pass may be NULL as in wz_detect_batch_fmt / wz_submit_device_fmt; host frames are staged whole and cropped from that
 * copy.  A tiled slot is collected like any other (wz_collect, or wz_wait + wz_slot_rows): n frames' merged rows.  Refused, with no row
 * written and nothing enqueued: n or the tiles of the call beyond max_batch, n_tiles[i] outside 1 .. WZ_MAX_TILES (WZ_ELIMIT); a
 * rectangle that is empty or leaves the frame, one the format cannot cut (NV12 / I420: even x0, y0, w, h; YUYV422 / UYVY422: even x0, w),
 * one wz_frame_bytes() refuses as a frame, a threshold that is NaN or negative (WZ_EINVAL).  The worker's frame table takes the same
 * rectangles per entry: wz_bind_tiles, below. */
#define WZ_MAX_TILES 64                       /* tiles of one frame */
typedef struct wz_tile { int32_t x0, y0, w, h; } wz_tile_t;   /* a rectangle of the frame, pixels */
int wz_detect_tiled(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt,
                    const int* cam, const int* n_tiles, const wz_tile_t* const* tiles, double iou_thr, double ios_thr,
                    wz_detection_t* const* out, uint8_t* const* pass, float* ms);
int wz_submit_tiled_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h,
                           const int* fmt, const int* cam, const int* n_tiles, const wz_tile_t* const* tiles,
                           double iou_thr, double ios_thr);      /* collected with wz_collect / wz_wait + wz_slot_rows */
/* ---- gated tiled detection.  A fixed camera shows an unchanged picture in most tiles most of the time.  A camera
 * whose tiles are set once (wz_set_camera_tiles) keeps, per tile and in device memory, a REFERENCE -- the sum of the lumas of every cell of
 * WZ_GATE_CELL x WZ_GATE_CELL pixels (anchored at the tile's origin; the last column and row of cells are partial) in the picture the
 * tile last ran on, uint16 a cell -- and the 100 rows the tile produced on that picture.  A gated call measures every tile of its frames
 * in one launch, runs the network on the tiles that drifted and gives the merge launch of a tiled call fresh rows for those and the
 * cached rows for the others; the result is what wz_detect_tiled defines, on those rows, in tile order, then the camera filter.
 *   luma of a pixel   on the bytes as stored (the colour flags of the format word play no part): GRAY8 the byte; NV12 / I420 the byte of
 *                     the luma plane -- the chroma planes are not read, a change of chroma alone is not seen; YUYV422 / UYVY422 the Y byte;
 *                     RGB24 / BGR24 (77 R + 150 G + 29 B + 128) >> 8
 *   changed cell      |S_now - S_ref| > pixel_thr * (pixels of the cell), in integers; a tile's activity = its number of changed cells
 *   a tile runs iff   it has no reference (first call, after wz_reset_camera_tiles, after its layout was set), or activity >= min_cells,
 *                     or max_age > 0 and it was skipped in the last max_age consecutive gated calls of its camera
 * Reference and cached rows of a tile are replaced together and only when the tile runs: the cached rows always describe the picture the
 * reference was taken from, and slow drift adds up against that picture until it crosses the threshold.  If no tile of a call runs, no
 * crop and no batch are launched; merge and filters still run.  WZ_EINCOMPLETE is reported by the call in which the short tile RAN; a
 * later call that reuses its rows returns WZ_OK.
 * wz_set_camera_tiles waits for every lane, checks the rectangles as a tiled call does (inside the width x height frame of format fmt, the
 * format's even-ness, none larger than max_width x max_height), n_tiles in 1 .. min(WZ_MAX_TILES, max_batch) (WZ_ELIMIT), pixel_thr
 * in 0 .. 255, min_cells >= 1, max_age >= 0 (WZ_EINVAL) and allocates the camera's state; on failure the camera keeps the layout it had.
 * A gated call is refused, with nothing enqueued, no row written and no state changed: cam NULL, a camera id of -1 or without a layout,
 * a frame whose size or base format differs from the layout's, the same camera twice in one call, thresholds a tiled call refuses
 * (WZ_EINVAL); the cameras' CONFIGURED tile counts summing to more than max_batch (WZ_ELIMIT) -- never the running ones: a refusal does
 * not depend on pixels.  wz_submit_gated_device returns once the decision is made: it waits for the activity launch of its own lane and
 * for any other lane still running a gated batch of one of its cameras; everything behind stays asynchronous and the slot is collected
 * like any tiled slot.  wz_gate_stats: what the last gated call accepted on `slot` decided, for its n frames. */
#define WZ_GATE_CELL 16
typedef struct wz_tile_gate { int32_t pixel_thr, min_cells, max_age, _reserved; } wz_tile_gate_t;
int wz_set_camera_tiles(wz_engine_t* e, int cam, int width, int height, int fmt, int n_tiles, const wz_tile_t* tiles, const wz_tile_gate_t* gate);
int wz_reset_camera_tiles(wz_engine_t* e, int cam);   /* forget references and cached rows, keep the layout */
int wz_clear_camera_tiles(wz_engine_t* e, int cam);
int wz_detect_gated(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt, const int* cam,
                    double iou_thr, double ios_thr, wz_detection_t* const* out, uint8_t* const* pass, float* ms);
int wz_submit_gated_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt,
                           const int* cam, double iou_thr, double ios_thr);
int wz_gate_stats(wz_engine_t* e, int slot, int n, uint64_t* ran_mask /* [n], bit t: tile t ran */,
                  int32_t* activity /* [sum of tiles]; 0 for a tile without a reference; may be NULL */);
/* ---- motion regions.  The rectangles of a tiled or gated call are fixed in advance; a motion call finds them: it
 * cuts a rectangle at the camera's own resolution around every part of the picture that changed since the camera's previous motion
 * call -- plain frame differencing -- and runs the detector there, beside the squeezed whole frame if the camera asks for it.  The
 * activity launch of a gated call writes the whole frame's grid of WZ_GATE_CELL x WZ_GATE_CELL luma sums (cells and luma exactly as
 * above); a second launch, one workgroup per camera, turns the changed cells into at most WZ_MOTION_MAX_REGIONS ranked rectangles in
 * the lane's page-locked block; the host waits once, reads them, and everything behind is the tiled call on those rectangles.
 *   reference        the grid of the camera's previous ACCEPTED motion call, replaced on every accepted call (two grids per camera,
 *                    swapped by pointer).  Without one -- first call, after wz_reset_camera_motion, after wz_set_camera_motion --
 *                    no cell has changed.  A camera's motion state shares nothing with its gate tiles; it may have both.
 *   changed cell     C = 1 iff |S_now - S_ref| > pixel_thr * (pixels of the cell)
 *   dilation         D = 1 iff some C = 1 lies within `dilate` cells in x and in y
 *   components       the 8-connected components of D; id = the smallest y * columns + x of its cells, weight n = its cells with C = 1
 *                    (dilated cells do not count), cell box = the bounding box of its D cells
 *   candidates       the components with n >= min_cells by n descending, then id ascending; the first 64 are looked at
 *   the walk         in that order.  Tight rectangle: the cell box in pixels, clipped to the frame, grown by `pad` on every side and
 *                    clipped again.  A candidate whose tight rectangle lies wholly inside the FINAL rectangle of a region already
 *                    accepted is dropped.  Otherwise each axis is grown evenly to min(min_side, frame) pixels (the odd pixel goes
 *                    right / down) and shifted back into the frame; for NV12 / I420 / P010 / YUV420P10 x0, y0 go down and x1, y1 up
 *                    to even numbers (clipped), for YUYV422 / UYVY422 x0 and x1; the rectangle is accepted; max_regions end the walk.
 *   tile list        [the whole frame, if whole_frame] + the regions in the order they were accepted
 *   result           bit for bit what ONE wz_detect_tiled call of the same frames with these tile lists gives.  A frame whose list is
 *                    empty (whole_frame 0, nothing moved) gets the engine's 100 padding rows and pass bytes 0 whatever its camera's
 *                    filter says; if no frame of a call has a tile neither a crop nor a batch is launched.
 * wz_set_camera_motion waits for every lane and allocates the camera's two grids; on failure the camera keeps what it had.  Refused
 * with WZ_EINVAL: pixel_thr outside 0 .. 255, min_cells < 1, dilate outside 0 .. 2, max_regions outside 1 .. WZ_MOTION_MAX_REGIONS,
 * min_side < 16, pad outside 0 .. 64, whole_frame other than 0 / 1, a size or format wz_frame_bytes() refuses; with WZ_ELIMIT: a frame
 * larger than max_width x max_height, more than WZ_MOTION_MAX_CELLS cells, whole_frame + max_regions > max_batch.
 * A motion call is refused, with nothing enqueued, no row written and no state changed: cam NULL, a camera id of -1 or without
 * settings, a frame whose size or base format differs from the settings', the same camera twice, thresholds a tiled call refuses
 * (WZ_EINVAL); the CONFIGURED whole_frame + max_regions of the call's cameras summing to more than max_batch (WZ_ELIMIT) -- never the
 * regions found: a refusal does not depend on pixels.  wz_submit_motion_device returns once the rectangles are read: both
 * launches that touch the grids have finished by then, so no lane ever holds the motion state of a camera WITHOUT A HOLD (below) in
 * flight; the slot is collected like any tiled slot.  wz_motion_stats: what the last motion call accepted on `slot` found for its n
 * frames. */
#define WZ_MOTION_MAX_REGIONS 16
#define WZ_MOTION_MAX_CELLS   32768
typedef struct wz_motion { int32_t pixel_thr, min_cells, dilate, max_regions, min_side, pad, whole_frame, _reserved; } wz_motion_t;
int wz_set_camera_motion(wz_engine_t* e, int cam, int width, int height, int fmt, const wz_motion_t* motion);
int wz_reset_camera_motion(wz_engine_t* e, int cam);    /* forget the reference, keep the settings */
int wz_clear_camera_motion(wz_engine_t* e, int cam);
int wz_detect_motion(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt, const int* cam,
                     double iou_thr, double ios_thr, wz_detection_t* const* out, uint8_t* const* pass, float* ms);
int wz_submit_motion_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt,
                            const int* cam, double iou_thr, double ios_thr);
int wz_motion_stats(wz_engine_t* e, int slot, int n, int32_t* n_tiles /* [n] */, wz_tile_t* tiles /* [n][1 + WZ_MOTION_MAX_REGIONS] */,
                    int32_t* cells /* [n][WZ_MOTION_MAX_REGIONS]: n of every region */, int32_t* components /* [n]: those with n >= min_cells */);
/* ---- motion hold.  Frame differencing forgets: a person who stops moving leaves the regions one call later, and
 * what never moved never gets one.  A camera with motion settings may ALSO have a hold: a grid G of ages, one byte per cell of the same
 * 16 x 16-pixel cells, in device memory; all zero at first, after wz_reset_camera_motion and after new hold settings.  On every ACCEPTED
 * motion call of the camera, with C the changed cells as above (all 0 without a reference):
 *   active cells     A = C or (G > 0).  Regions, every region's n and `components` are exactly those above with A in the place of C (D is
 *                    A dilated, n counts the A cells of a component): a call without a reference can have regions, where G > 0.
 *   decay            G1 = max(hold if C else 0, G - 1 if G > 0 else 0)
 *   stamp            behind the merge, the camera filter and the padding rows: for every one of the frame's 100 merged rows whose final
 *                    pass byte is 1, with x0 = max(x_min, 0), x1 = min(x_max, width - 1) and the same in y, unless x0 > x1 or y0 > y1,
 *                    every cell with x0 >> 4 <= cx <= x1 >> 4 and y0 >> 4 <= cy <= y1 >> 4 gets G2 = max(G1, object_hold).  With
 *                    object_hold = 0 nothing is stamped.  What passes is what the camera's filter lets pass: confidence, area, zones.
 *   next call        G2 is its G.  A refused call changes nothing.
 * So a changed cell stays active for `hold` further calls, a cell under a passing detection for `object_hold` further calls, refreshed
 * while the detection recurs.  The rows of a call are, as before, one wz_detect_tiled call on the reported tile lists.
 * wz_set_camera_motion_hold waits for every lane and allocates the camera's two age grids (swapped like its two luma grids); on failure
 * the camera keeps what it had; hold = object_hold = 0 removes the hold and frees them.  Refused with WZ_EINVAL: a null argument, a
 * camera without motion settings, a value outside 0 .. 255.  wz_set_camera_motion replaces the camera and thereby DROPS its hold: set
 * the hold after it.  An engine that never sets a hold allocates nothing for it, and the calls of a camera without one launch and wait
 * for nothing more than before.
 * In flight: the stamp launch of a camera with a hold is still running when wz_submit_motion_device returns.  The next motion call of that
 * camera on ANOTHER lane waits for the lane that stamped it before it launches anything (as a gated call does for its camera's commit
 * launch); on the same lane the stream orders them.
 * wz_motion_hold_stats: per frame of the last motion call accepted on `slot`, its active cells and those of them that did not change
 * (active - held changed); 0 and 0 for a frame whose camera has no hold. */
typedef struct wz_motion_hold { int32_t hold, object_hold, _reserved[2]; } wz_motion_hold_t;
int wz_set_camera_motion_hold(wz_engine_t* e, int cam, const wz_motion_hold_t* hold);   /* both 0: remove the hold, free its grids */
int wz_motion_hold_stats(wz_engine_t* e, int slot, int n, int32_t* active /* [n] */, int32_t* held /* [n] */);
/* ---- ignore masks.  A real camera burns a clock into its picture, shows a flag, a hedge in the wind, a road behind
 * the fence: pixels that change on every frame and are no motion.  A camera with motion settings, a gate layout or both may have one IGNORE
 * PLANE: height x width bytes, nonzero = ignore.  From it the engine derives one bit per 16 x 16-pixel cell of every grid the camera
 * compares; a changed cell whose bit is set does not count.  Nothing else about a call changes.
 *   cell rule   a cell is ignored iff AT LEAST ONE pixel of it is ignored in the plane.  A cell is WZ_GATE_CELL square; the last column and row
 *               of cells of a grid are partial.  What was painted never leaks as motion; the price is a margin of at most 15 pixels around the
 *               painted area in which change is ignored too.  A motion camera's grid is anchored at the frame's origin.  A gated camera has
 *               one grid per tile, anchored at the TILE's origin: tile origins need not be multiples of 16, so a tile's cell bits are derived
 *               from the plane for that tile and are not a window of the frame's.  wz_ignore_cells is the one place the rule is written.
 *   motion      with C the changed cells as defined above and M the ignored cells, C' = C and not M.  Every later definition reads C' where it
 *               reads C: dilation, components, a region's n, candidates, the walk.  With a hold: A = C' or (G > 0), and the decay uses C' -- an
 *               ignored cell never receives `hold` from change.  The stamp is untouched: a cell under a passing detection is held even if it
 *               is ignored (the mask silences change, not the detector's findings), and such a cell stays active while its age lasts.  The
 *               grid of luma sums is written and becomes the next call's reference as before, ignored cells included.
 *               ignored = |C and M|, the changed cells that the mask removed; 0 without a reference.
 *   gate        a tile's activity is its number of changed cells that are not ignored.  "A tile runs iff" is unchanged in every other clause:
 *               no reference, max_age, min_cells.  wz_gate_stats' activity is the count after masking.
 *   no mask     a camera without a mask behaves bit for bit as before, and a call none of whose cameras has one launches the kernels it
 *               launched before there were masks.
 * wz_ignore_cells: host only, no engine needed.  cells[cell rows][cell columns] of `rect` (NULL: the whole frame) get 0 / 1.  WZ_EINVAL: a
 * null plane or output, a size below 1, a rect that is empty or not inside the frame.
 * wz_set_camera_ignore waits for every lane and applies to what the camera has at the time of the call: its motion settings get the frame
 * grid's bits, its gate layout every tile's bits.  Refused with WZ_EINVAL: a camera that has neither; a plane whose size differs from the
 * size either was set for.  On failure the camera keeps what it had.  ignore = NULL removes the mask (width and height are not looked at).
 * The lifecycle follows the hold's: wz_set_camera_motion replaces the camera's motion state and thereby drops the motion part of the mask,
 * wz_set_camera_tiles the gate part -- set the mask after them (wz_set_camera_motion_hold keeps it); wz_reset_camera_* keeps the mask;
 * wz_clear_camera_* frees its part.  An engine that never sets a mask allocates nothing for it.
 * wz_motion_ignore_stats: per frame of the last motion call accepted on `slot`, the changed cells that the mask removed; 0 for a frame whose
 * camera has no mask.  The frame-table path (wz_bind_tiles(..., gated = 1) + wz_submit_bound) looks the camera's layout up at submit time and
 * honours the mask like wz_detect_gated. */
int wz_ignore_cells(const uint8_t* ignore, int width, int height, const wz_tile_t* rect /* NULL: the whole frame */,
                    uint8_t* cells /* [cell rows][cell columns], 0 / 1 */);
int wz_set_camera_ignore(wz_engine_t* e, int cam, int width, int height, const uint8_t* ignore /* [height][width], nonzero: ignore; NULL: remove */);
int wz_motion_ignore_stats(wz_engine_t* e, int slot, int n, int32_t* ignored /* [n] */);
/* ---- the worker's frame table.  The reference worker resolves every payload to `frame_buffers[sender].frames[index]`, asks
 * the frame for a numpy view of its pixels and hands the frame header's `Detection[100]` array to the plugin
 * (watsor/detection/detector.py:102-109); pixels, size and rows of a Frame never move after the FrameBuffers are created
 * (watsor/stream/share.py:27-41,76-81).  So they are described ONCE (entry i = one Frame: pixels, w, h, WZ_FMT_*, camera id or
 * -1, its rows), a batch is then n table indices, and the rows land in the frames' own headers.  fmt / cam may be NULL (RGB24 /
 * no camera).  The pixels travel as wz_submit_host moves them (one copy per frame on the lane's stream: DMA from
 * wz_host_register()ed memory).  wz_bind_frames replaces the whole table (waits for the lanes first) and with it every tiled
 * description wz_bind_tiles gave its entries. */
int wz_bind_frames(wz_engine_t* e, int n, const uint8_t* const* pixels, const int* w, const int* h, const int* fmt,
                   const int* cam, wz_detection_t* const* rows);
/* Tiled and gated detection through the frame table: entries first .. first + count - 1 of the current table --
 * normally the frames of one camera's FrameBuffer -- get a tiled description.  Waits for every lane first; on any refusal no entry changes.
 *   gated == 0, n_tiles >= 1   tiles[0 .. n_tiles) are the entries' rectangles, iou_thr / ios_thr their merge thresholds (wz_detect_tiled).
 *                              Checked against EVERY entry's own width, height and format word as a tiled call checks them (inside the
 *                              frame, the format's even-ness, none larger than max_width x max_height: WZ_EINVAL / WZ_ELIMIT); n_tiles
 *                              outside 1 .. min(WZ_MAX_TILES, max_batch): WZ_ELIMIT; a threshold that is NaN or negative: WZ_EINVAL.
 *   gated != 0                 tiles must be NULL and n_tiles 0 (WZ_EINVAL): rectangles and gate are the ones wz_set_camera_tiles gave the
 *                              entries' camera -- all entries of the range must carry the same camera id >= 0 (WZ_EINVAL).  The layout is
 *                              looked up when a batch is submitted: it may be set or replaced after this call.
 *   gated == 0, n_tiles == 0, tiles == NULL   the entries are untiled again.
 * first / count outside the table: WZ_EINVAL. */
int wz_bind_tiles(wz_engine_t* e, int first, int count, int n_tiles, const wz_tile_t* tiles, double iou_thr, double ios_thr, int gated);
/* Motion regions through the frame table: entries first .. first + count - 1 of the current table -- the frames of one
 * motion camera's FrameBuffer -- get a motion description with the merge thresholds iou_thr / ios_thr (wz_detect_motion).  It carries no
 * rectangles and no settings: settings, hold and ignore mask are the ones wz_set_camera_motion, wz_set_camera_motion_hold and
 * wz_set_camera_ignore gave the entries' camera, looked up when a batch is submitted -- they may be set or replaced after this call.  Waits
 * for every lane first; on any refusal no entry changes.  WZ_EINVAL: a null engine; first / count outside the table; entries that do not all
 * carry one camera id >= 0; a threshold that is NaN or negative.  wz_bind_tiles(e, first, count, 0, NULL, .., 0) makes the entries untiled
 * again; wz_bind_frames drops the descriptions with the table. */
int wz_bind_motion(wz_engine_t* e, int first, int count, double iou_thr, double ios_thr);
/* A batch of table entries on lane `slot`.  All entries untiled: an ordinary batch, as wz_submit_host runs it.  All entries tiled: the
 * tiled call wz_detect_tiled defines, with every refusal of one (the tiles of the batch beyond max_batch: WZ_ELIMIT; a camera filter set
 * for another size: WZ_EINVAL), made before anything is enqueued; the entries' thresholds must be equal (WZ_EINVAL: the merge launch takes one pair).  All entries
 * gated: the gated call wz_detect_gated defines, with its refusals (one frame per camera and call, a camera without a layout or with one
 * of another size or base format: WZ_EINVAL; the configured tile counts beyond max_batch: WZ_ELIMIT) and equal thresholds; the call
 * returns once the decision is made, as wz_submit_gated_device does, and wz_gate_stats describes the slot.  All entries motion
 * (wz_bind_motion): the motion call wz_detect_motion defines, with its refusals (one frame per camera and call, a camera without motion
 * settings or with settings of another size or base format: WZ_EINVAL; the cameras' configured whole_frame + max_regions beyond max_batch:
 * WZ_ELIMIT) and equal thresholds; the call returns once the rectangles are read, as wz_submit_motion_device does, and wz_motion_stats,
 * wz_motion_hold_stats and wz_motion_ignore_stats describe the slot.  A batch that mixes two of the four kinds: WZ_EINVAL.  A refusal
 * leaves the lane, the cameras' gate and motion state and every row as they were.
 * Where the pixels of a tiled or gated entry come from: a frame inside a wz_host_register()ed range is read IN PLACE by the crop and
 * activity kernels (which read the rectangles' rows and nothing else) when the rectangles' bytes -- wz_frame_bytes(tile w, tile h, fmt)
 * summed over the frame's tiles, twice that for a gated entry, whose tiles are measured and then read again when they run -- are at
 * most half of the frame's; otherwise the frame is staged whole by one DMA and cut from that copy.  A motion entry is always staged
 * whole: its activity launch reads every luma pixel of the frame, so what it reads is never at most half of the frame's bytes. */
int wz_submit_bound(wz_engine_t* e, int slot, int n, const int32_t* entries);
/* waits for `slot`, writes its rows into the bound frames' rows: the batch's own rows or, after a tiled or gated submit, the frames'
 * merged rows (also when no tile of a gated batch ran, and when no frame of a motion batch had a tile: padding rows).  WZ_EINCOMPLETE is returned after the rows are written, as by wz_collect. */
int wz_collect_bound(wz_engine_t* e, int slot);
/* Wait for `slot` without copying rows out (rows stay readable via wz_slot_rows). */
int wz_wait(wz_engine_t* e, int slot);
const wz_detection_t* wz_slot_rows(wz_engine_t* e, int slot); /* pinned host, [n][100]; after a tiled submit: the n frames' merged rows */
int wz_sync(wz_engine_t* e);
int wz_graph_nodes(wz_engine_t* e, int slot);   /* nodes of the hipGraph last replayed on `slot` (kernel launches; no copy node unless the lane's descriptor block has no device address); 0 without graphs */
int wz_num_slots(wz_engine_t* e);   /* lanes actually created (WZ_SLOTS unless WZ_LANES in the environment says fewer) */

/* ---- per-camera filters on the GPU: ConfidenceFilter / AreaFilter / MaskFilter
 * (watsor/filter/confidence.py:10-19, area.py:10-26, mask.py:17-59).
 *   conf_thr[l]  confidence/100 for label l, NaN when the label is not configured (-> reject)
 *   area_thr[l]  area/100 * (width*height) as the reference computes it, NaN when not configured
 *   n_zones      number of zones of the camera's mask (0 = no mask -> Mask filter absent)
 *   zone_allow   [WZ_NUM_LABELS][n_zones] bytes: 1 if label l may report zone z (mask.py:29-42);
 *                NULL = every label sees every zone
 *   zone_fill    [n_zones][height][width] bytes: 1 on the lattice points of zone z's polygon
 *                (8-connected alpha==255 component with holes filled, ordered as mask.py:78-88)
 * n_zones == 0 with zone_fill != NULL: a mask IS configured but holds no zone -- every row then fails the mask test,
 * as the reference's MaskFilter with an empty polygon list does (mask.py:44-59); n_zones == 0 with zone_fill == NULL:
 * no mask.  On failure the camera keeps the filter it had.
 */
int wz_set_camera_filter(wz_engine_t* e, int cam, int width, int height, const double* conf_thr,
                         const double* area_thr, int n_zones, const uint8_t* zone_allow,
                         const uint8_t* zone_fill);
int wz_clear_camera_filter(wz_engine_t* e, int cam);
/* Drop mode for a camera that has a filter: rows that fail `label > 0 and Confidence and Area and Mask`
 * (watsor/filter/track.py:26) are written as all-zero rows, so that whatever reads the frame's detections next
 * (the sieve's TrackFilter) rejects them by its own `label > 0` test and need not run the filters again. */
int wz_set_camera_drop(wz_engine_t* e, int cam, int drop);
/* Run only the filter stage on caller-provided rows (host), in place: zones are written into the
 * rows exactly where the reference's MaskFilter would have been invoked; pass[100] receives the verdict. */
int wz_filter_rows(wz_engine_t* e, int cam, wz_detection_t* rows, uint8_t* pass);

/* Host-side zone extraction from an alpha plane: MaskFilter.__init__ / find_contours / contours_key
 * (mask.py:17-27,78-88) without OpenCV.  Writes up to max_zones filled-zone bitmaps ([z][h][w] bytes)
 * ordered by the reference's centroid key and returns the zone count (or a negative error). */
int wz_zones_from_alpha(const uint8_t* alpha, int width, int height, int max_zones, uint8_t* zone_fill,
                        int32_t* centroid_xy /* [max_zones][2], may be NULL */);

/* ---- the sieve's tracker, host code, one instance per camera, no engine needed.
 * Replaces TrackFilter(filters, sensitivity, history) of watsor/filter/track.py:19-149 for rows whose per-detection
 * filters already ran on the GPU; row order, new-track order (CPython set iteration) and zone order of the combined
 * rows are the reference's; equally-near tracks are visited in index order (np.argsort's tie order is not defined). */
typedef struct wz_tracker wz_tracker_t;
int wz_tracker_create(int sensitivity, int history, wz_tracker_t** out);   /* track.py:19-23; defaults 5, 10 */
void wz_tracker_destroy(wz_tracker_t* t);
int wz_tracker_reset(wz_tracker_t* t);
int wz_tracker_count(wz_tracker_t* t);                                     /* live tracks, all labels */
/* TrackFilter.__call__ (track.py:25-110) on n rows; a row takes part iff label > 0 and (pass == NULL or pass[i]).
 * Writes min(*n_out, cap) combined rows (track.py:118-149) to out, *n_out = rows the reference would return,
 * *suspicious = its second return value (track.py:38). */
int wz_tracker_update(wz_tracker_t* t, const wz_detection_t* rows, int n, const uint8_t* pass, wz_detection_t* out,
                      int cap, int* n_out, int* suspicious);
/* DetectionSieve._incoming_frame (watsor/filter/sieve.py:21-33,44-56) with one TrackFilter, in place on the
 * frame header's rows: results first, the remaining rows zeroed. */
int wz_tracker_sieve(wz_tracker_t* t, wz_detection_t* rows, int n, const uint8_t* pass, int* suspicious);
/* ---- what the engine file holds (read once by HipEngine.__init__) */
int wz_input_size(wz_engine_t* e);
int wz_num_anchors(wz_engine_t* e);
int wz_num_classes(wz_engine_t* e);
int wz_precision(wz_engine_t* e);   /* 16: fp16 storage / fp16 MFMA; 32: fp32 storage / exact-fp32 MFMA (engine built with -p 32) */
/* leading inverted-residual blocks that run with split (hi + lo) matrix operands; 0 = plain fp16 program
 * (`python -m watsor_amd.engine --plain-fp16`), whose scores miss the 1e-3 tolerance */
int wz_hp_blocks(wz_engine_t* e);
double wz_nms_iou(wz_engine_t* e);  /* the IoU threshold of the engine's own non-maximum suppression (what a tiled call merges with by default) */

/* ---- device memory helpers so callers need no other GPU runtime binding
 * Every synchronous copy or fill of the product ABI -- these two, engine creation, the camera-filter setters, the first gated call of a
 * lane -- is issued on lane 0's stream and waited for there (never on the null stream, whose hardware queue a process that uses only
 * this ABI therefore never opens): a call made while lane 0 has a batch in flight returns after that batch.  The copy is complete
 * and the host buffer free when the call returns; the other lanes are not waited for. */
int wz_dev_alloc(wz_engine_t* e, uint64_t bytes, void** d_ptr);
int wz_dev_free(wz_engine_t* e, void* d_ptr);
int wz_dev_upload(wz_engine_t* e, void* d_dst, const void* h_src, uint64_t bytes);
int wz_dev_download(wz_engine_t* e, void* h_dst, const void* d_src, uint64_t bytes);

/* ======================================================================================================================
 * Development library only (`make dev` -> libwatsor_hip_dev.so, compiled with -DWZ_DEV_BUILD): stage-level entry points of the
 * parity tests, per-kernel profiling for bench.py's roofline, diagnostics, and -- inside the library -- the WZ_* tuning knobs and
 * the kernel variants that lost their A/B (HISTORY.md part B).  libwatsor_hip.so exports nothing below this line and reads
 * only WZ_LANES, WZ_STREAMS, WZ_GRAPH and WZ_SCHEDULE from the environment.
 * ====================================================================================================================== */
#ifdef WZ_DEV_BUILD
/* Test hooks for the CPython-set emulation: iteration order after adding keys[0..n) / of
 * `set(range(n)).difference(used)`; both return the number of values written to out. */
int wz_debug_pyset_order(const int32_t* keys, int n, int32_t* out);
int wz_debug_unused_order(int n, const uint8_t* used, int32_t* out);

/* ---- introspection used by bench.py (roofline) and the parity tests */
int wz_num_tensors(wz_engine_t* e);
int wz_tensor_info(wz_engine_t* e, int idx, char* name, int namelen, int* h, int* w, int* c);
/* bit 0: the tensor is stored as a hi + lo pair of halves per value (2c halves per pixel: c hi, then c lo) --
 * the tensors between the split-operand blocks of the `-p 16` program (csrc/k_mbconv_hp.hip) */
int wz_tensor_flags(wz_engine_t* e, int idx);
int wz_num_ops(wz_engine_t* e);
/* dims[12] = kind,cin,cout,ksize,stride,hin,win,hout,wout,n_pad,kc,splitk */
int wz_op_info(wz_engine_t* e, int idx, char* name, int namelen, int* dims);
int wz_num_stages(wz_engine_t* e);                              /* kernels per batch, pre + ops + post */
int wz_stage_name(wz_engine_t* e, int stage, char* name, int namelen);
/* Run the pipeline `reps` times on device frames with a hipEvent pair around every kernel launch
 * (events on the engine's own stream); stage_ms[stage] = mean milliseconds of that launch. */
int wz_profile_device(wz_engine_t* e, int n, const uint8_t* const* d_rgb, const int* w, const int* h,
                      int reps, float* stage_ms);
/* The same with every kernel of the pre-processing and the network enqueued `inner` times back to back inside its
 * bracket (they are pure functions of their inputs): stage_ms[stage] = mean milliseconds of the whole bracket, so
 * (stage_ms - empty bracket) / inner is a launch INCLUDING its in-stream boundary, with the cost of the event pair
 * amortised rather than estimated.  The post-processing stages run once. */
int wz_profile_stages(wz_engine_t* e, int n, const uint8_t* const* d_rgb, const int* w, const int* h,
                      int reps, int inner, float* stage_ms);

/* diagnostics: 16 words per frame written by the NMS kernel of lane 0 (phase timestamps at 100 MHz, counts) */
int wz_debug_nms(wz_engine_t* e, int n, uint64_t* out);
/* What the post-processing of the batch last run on lane `slot` left in device memory, read back after that batch was collected; no
 * kernel is launched.  n = frames of that batch (1 .. max_batch); any output pointer may be null.
 *   box_enc [n][A][4], logits [n][A][C]    the lane's head outputs
 *   boxes [n][T][4], scores [n][T], classes [n][T], num [n]    the det_* arrays of the lane's NMS kernel (T = max_total)
 *   dbg [n][16]    the lane's block of wz_debug_nms words: 8 = candidates of the first band, 9 = rows kept after it, 10 = candidates
 *                  walked in all, 14 = entries found in the candidate bit map (0: the first band was scanned), 15 = the first band's
 *                  lower bin as walked (low 32 bits), the hint on entry (bits 32 .. 47) and whether the exact serial walk of a crowded
 *                  bin ran (bit 48); the rest are timestamps
 *  Engines with max_total other than 100 are refused (the arrays are laid out [n][T]).
 *   flags [2]      {decode_fused, cands_listed} of the launches of that batch (0, 0 while the lane has run stage-level calls only) */
int wz_debug_post_lane(wz_engine_t* e, int slot, int n, float* box_enc, float* logits, float* boxes, float* scores,
                       int32_t* classes, int32_t* num, uint64_t* dbg, int32_t* flags);
/* Engines created with WZ_MB_DEBUG=1 in the environment: phase timestamps (100 MHz) of the first and the last
 * workgroup of every fused inverted-residual block, out[n_ops][16]; groups[n_ops] = channel groups launched. */
int wz_debug_mbconv(wz_engine_t* e, uint64_t* out, int32_t* groups);

/* Lane stamps -- only in a library built with -DWZ_LANE_STAMPS=1 (`make stamps` -> libwatsor_hip_stamps.so; elsewhere both return
 * WZ_EINVAL): every kernel of a batch records when its first workgroup entered and its last one left (100 MHz ticks of the
 * device's constant clock).  After wz_wait(slot): out[2k], out[2k+1] = entry / exit of launch k of that batch (launch 0 = the resize
 * kernel, the last one = the NMS kernel); returns the number of launches.  wz_debug_lane_launch: kernel name and
 * dims[5] = {workgroups, threads per workgroup, LDS bytes, workgroups one CU holds, registers} of launch idx; returns the number of
 * launches.  What tools/lane_overlap.py turns into kernels-in-flight and CU-slot-time per step without a profiler in the way. */
int wz_debug_lane_stamps(wz_engine_t* e, int slot, uint64_t* out, int cap);
int wz_debug_lane_launch(wz_engine_t* e, int slot, int idx, char* name, int namelen, int* dims);

/* ---- stage-level entry points for the parity tests (host in, host out, synchronous) */
/* resize + normalise of one frame -> half[size*size*4] (x,y,z,0 per pixel); when the input tensor is a pair
 * (wz_tensor_flags) half[size*size*8]: (x,y,z,0) hi then (x,y,z,0) lo per pixel */
int wz_stage_preprocess(wz_engine_t* e, const uint8_t* rgb, int w, int h, uint16_t* out_half);
int wz_stage_preprocess_fmt(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, uint16_t* out_half);
/* network only: half input [n][size][size][4] -> float box encodings [n][A][4], logits [n][A][C]
 * (a pair input tensor gets these halves as its hi parts and zeros as its lo parts) */
int wz_stage_forward(wz_engine_t* e, int n, const uint16_t* in_half, float* box_enc, float* logits);
/* read activation tensor `idx` of frame `frame` left behind by the last forward (half, NHWC; a pair tensor
 * comes back as stored, 2c halves per pixel).
 * Only meaningful when the engine was created with WZ_NO_BUFFER_REUSE=1 in the environment. */
int wz_stage_read_tensor(wz_engine_t* e, int idx, int frame, uint16_t* out_half);
/* one fused block (op `op` of wz_op_info) of the last forward again, for its n frames, with its source tensor read at the device
 * address `d_in` (wz_dev_alloc / wz_dev_upload: n frames as wz_stage_read_tensor returns them, back to back) -- the caller decides
 * what lies in front of and behind the tensor.  The block's outputs land where the network puts them.  launch_frames > 0: a
 * split-operand block goes out as launches of at most that many frames (what a batch of 2^31 bytes of block input and more gets);
 * 0: as the network launches it. */
int wz_stage_block_at(wz_engine_t* e, int op, int n, const void* d_in, int launch_frames);
/* decode + sigmoid + NMS + top-k on caller-provided head outputs:
 * boxes [n][100][4] (ymin,xmin,ymax,xmax), scores [n][100], classes [n][100] (1-based), num [n] */
int wz_stage_postprocess(wz_engine_t* e, int n, const float* box_enc, const float* logits, float* boxes,
                         float* scores, int32_t* classes, int32_t* num);
/* The post-processing of a real batch on caller-provided head outputs, on lane 0: the values enter as the partial sums of the grouped
 * head reduce (one K slice, zero bias: they come out bit for bit), which stores them, decodes the boxes and marks the candidates against
 * the lane's hint; the NMS kernel then reads its first band from that bit map and writes rows [n][100] for frames of size w x h -- the
 * launches of wz_submit_* behind the head convolutions.  wz_debug_post_lane(e, 0, n, ...) reads back what they left. */
int wz_stage_post_production(wz_engine_t* e, int n, const float* box_enc, const float* logits, int w, int h, wz_detection_t* rows);
/* row fill (tensorflow_cpu.py:79-90) for caller-provided detections of one frame of size w x h */
int wz_stage_rows(wz_engine_t* e, int w, int h, const float* boxes, const float* scores,
                  const int32_t* classes, wz_detection_t* rows);
/* tiled detection, stage by stage: one rectangle of one host frame through the crop kernel -> out[wz_frame_bytes(tile->w, tile->h, fmt)]
 * (byte for byte the contiguous copy of the same slices) ... */
int wz_stage_crop_tile(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, uint8_t* out);
/* ... and the merge kernel + camera filter on caller-provided rows of the tiles of one w x h frame (cam: a camera id or -1) */
int wz_stage_merge_tiles(wz_engine_t* e, int w, int h, int cam, int n_tiles, const wz_tile_t* tiles,
                         const wz_detection_t* tile_rows /* [n_tiles][100] */, double iou_thr, double ios_thr,
                         wz_detection_t* rows /* [100] */, uint8_t* pass /* [100] */);
/* HIP-event time (ms, mean of reps) of the crop launch alone and of the merge launch alone, behind one tiled call of these arguments on lane 0;
 * empty_ms: the same pair of event records with nothing between them */
int wz_profile_tiled(wz_engine_t* e, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt,
                     const int* n_tiles, const wz_tile_t* const* tiles, double iou_thr, double ios_thr, int reps,
                     float* crop_ms, float* merge_ms, float* empty_ms);
/* the activity kernel on one rectangle of one host frame, synchronous: sums_out[cell rows][cell columns] (uint16) and, against the grid `ref`
 * (NULL: no reference, 0 changed), the number of changed cells */
int wz_stage_tile_activity(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, const uint16_t* ref, int pixel_thr,
                           uint16_t* sums_out, int32_t* changed_out);
/* HIP-event time (ms, mean of reps) of the activity launch alone and of the commit launch alone, as one gated call of these arguments on lane 0
 * issued them (the call runs first, with whatever state its cameras have); empty_ms: the same bracket around nothing */
int wz_profile_gated(wz_engine_t* e, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt, const int* cam,
                     double iou_thr, double ios_thr, int reps, float* activity_ms, float* commit_ms, float* empty_ms);
/* the region kernel alone on two caller-provided grids ([cell rows][cell columns] uint16 of a w x h frame of format fmt; ref NULL: no
 * reference), synchronous: the regions in the order they were accepted, every region's n, the components with n >= min_cells */
int wz_stage_motion_regions(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* motion,
                            int32_t* n_regions, wz_tile_t* regions /* [WZ_MOTION_MAX_REGIONS] */, int32_t* cells /* [WZ_MOTION_MAX_REGIONS] */,
                            int32_t* components);
/* HIP-event time (ms, mean of reps) of the region launch alone on these two grids, and of the whole-frame activity launch of a w x h frame
 * of format fmt (device memory of undefined content) alone; empty_ms: the same bracket around nothing */
int wz_profile_motion(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* motion, int reps,
                      float* regions_ms, float* activity_ms, float* empty_ms, int32_t* rounds /* rounds of the labelling; 0: no changed cell */);
/* the region kernel alone as a camera with a hold runs it: wz_stage_motion_regions plus the ages age_in ([cell rows][cell columns] uint8;
 * NULL: all zero) and `hold` (0 .. 255); ref NULL: no cell has changed.  Also returns the active cells, those of them that did not change,
 * and the decayed ages age_out[cell rows][cell columns] */
int wz_stage_motion_hold(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, const uint8_t* age_in, int w, int h, int fmt,
                         const wz_motion_t* motion, int hold, int32_t* n_regions, wz_tile_t* regions /* [WZ_MOTION_MAX_REGIONS] */,
                         int32_t* cells /* [WZ_MOTION_MAX_REGIONS] */, int32_t* components, int32_t* active, int32_t* held, uint8_t* age_out);
/* the stamp kernel alone on the ages of a w x h frame, 100 rows and their 100 pass bytes: age_out = the ages behind it */
int wz_stage_motion_stamp(wz_engine_t* e, const uint8_t* age_in, const wz_detection_t* rows /* [100] */, const uint8_t* pass /* [100] */, int w, int h,
                          int object_hold, uint8_t* age_out);
/* waits for every lane, then copies the current age grid of camera `cam` ([cell rows][cell columns] uint8); WZ_EINVAL if it has no hold */
int wz_debug_motion_age(wz_engine_t* e, int cam, uint8_t* out);
/* HIP-event time (ms, mean of reps) of the region launch alone with these ages (age_in NULL: all zero) and of the stamp launch alone on the
 * ages it leaves, with these 100 rows and pass bytes; empty_ms: the same bracket around nothing */
int wz_profile_motion_hold(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, const uint8_t* age_in, int w, int h, int fmt,
                           const wz_motion_t* motion, int hold, const wz_detection_t* rows, const uint8_t* pass, int object_hold, int reps,
                           float* regions_ms, float* stamp_ms, float* empty_ms);
/* ---- ignore masks: the kernels' masked instantiations alone.  cells_ignored: [cell rows][cell columns] bytes as
 * wz_ignore_cells writes them (nonzero: ignored), or NULL: the camera / tile has no mask but runs in a launch that has one.
 * The activity kernel: wz_stage_tile_activity's arguments plus the tile's cell mask; changed_out counts the changed cells that are not ignored */
int wz_stage_tile_activity_ignore(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, const uint16_t* ref, int pixel_thr,
                                  const uint8_t* cells_ignored, uint16_t* sums_out, int32_t* changed_out);
/* the region kernel: wz_stage_motion_hold's arguments plus the grid's cell mask in and `ignored` out.  age_out NULL (then age_in NULL and
 * hold 0): as a camera without a hold runs it; active and held are then 0 */
int wz_stage_motion_ignore(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, const uint8_t* age_in, int w, int h, int fmt,
                           const wz_motion_t* motion, int hold, const uint8_t* cells_ignored, int32_t* n_regions,
                           wz_tile_t* regions /* [WZ_MOTION_MAX_REGIONS] */, int32_t* cells /* [WZ_MOTION_MAX_REGIONS] */, int32_t* components,
                           int32_t* active, int32_t* held, int32_t* ignored, uint8_t* age_out);
/* HIP-event time (ms, mean of reps) of the region launch alone on these two grids with this cell mask (no hold); empty_ms: the same
 * bracket around nothing.  The masked activity launch is timed by wz_profile_gated on a camera that has a mask */
int wz_profile_motion_ignore(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* motion,
                             const uint8_t* cells_ignored, int reps, float* regions_ms, float* empty_ms);
/* in_place[i] = 1 where frame i of the last wz_submit_bound on `slot` -- untiled, tiled or gated -- was read in place through its device view,
 * 0 where it was staged by DMA (n values: the frames of that batch; every frame of a motion batch: 0); WZ_EINVAL when the lane has seen no
 * such batch */
int wz_debug_bound_source(wz_engine_t* e, int slot, int32_t* in_place /* [n] */);

#endif /* WZ_DEV_BUILD */

#ifdef __cplusplus
}
#endif
#endif /* WATSOR_HIP_H */
