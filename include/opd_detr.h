/*
 * opd_detr.h — C-ABI of the MI355X-native DETR person-detection forward pass (libopd_hip.so).
 *
 * The reference (Kizuna42/office-person-detection-vit) is 100 % Python and has no FFI: its Phase-2 detector is a
 * Python class wrapping Hugging Face `DetrForObjectDetection` (deleted `src/detection/vit_detector.py`, method map
 * in `coverage.json:1`; today's stand-in with the same surface is `src/detection/yolov8_detector.py:19-254`).  The
 * entry points below are what a ctypes binding of that class would call; each one names the reference interface it
 * replaces.  Plain pointers and sizes only — no torch / numpy types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success or a negative OPD_E* code; it never throws and never aborts.  The
 *     human-readable reason of the last failure on the calling thread is `opd_last_error()`.  The Python shim turns a
 *     non-zero code into `RuntimeError`, which preserves the reference's conventions: load failure ->
 *     RuntimeError("Failed to load ... model: ...") (`yolov8_detector.py:86-88`), inference errors re-raised
 *     (`:130-132`) and converted to an empty detection list by the phase (`src/pipeline/phases/detection.py:124-127`).
 *   - output buffers are caller-allocated; the library owns only the model, its workspace and its HIP stream.
 *   - single caller at a time per handle (the reference is strictly single-threaded).  DIFFERENT handles may
 *     be driven from different threads at once (throughput mode: several handles per GPU); the library serialises the one
 *     operation that needs it, hipGraph capture, internally.
 *   - tensors: logits [B][Q][C+1] f32, boxes [B][Q][4] f32 (cx,cy,w,h in [0,1]), encoder features [B][h*w][D] f32
 *     with h = ceil(H/32), w = ceil(W/32) (HF `DetrObjectDetectionOutput`: logits, pred_boxes,
 *     encoder_last_hidden_state; HF:models/detr/modeling_detr.py:1329-1443).
 */
#ifndef OPD_DETR_H
#define OPD_DETR_H

#include <stddef.h>
#include <stdint.h>

/* The product library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#if defined(__GNUC__)
#define OPD_API __attribute__((visibility("default")))
#else
#define OPD_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define OPD_OK 0
#define OPD_EINVAL (-1)   /* bad argument (null pointer, shape out of the configured maximum, ...) */
#define OPD_EIO (-2)      /* weight file missing / unreadable / malformed */
#define OPD_ESCHEMA (-3)  /* weight file lacks a tensor of the DETR state dict or has the wrong shape */
#define OPD_EHIP (-4)     /* a HIP runtime call failed (message carries hipGetErrorString) */
#define OPD_ENOMEM (-5)   /* device or host allocation failed */
#define OPD_ESTATE (-6)   /* call not valid in the handle's current state */

typedef struct opd_detr opd_detr; /* opaque model handle */

/* Input pixel formats accepted by the forward entry points. */
#define OPD_PIXELS_U8_BGR_HWC 0 /* the reference's frame: numpy uint8 [H][W][3], BGR (`yolov8_detector.py:90-96`) */
#define OPD_PIXELS_F32_NCHW 1   /* HF `pixel_values`: float32 [B][3][H][W], already normalised */

/* Where the caller's buffers live. */
#define OPD_MEM_HOST 0
#define OPD_MEM_DEVICE 1 /* pointers are HIP device pointers on the handle's device */
#define OPD_MEM_HOST_PIXELS_DEVICE_OUT 2 /* pixels in host memory, every output pointer a device pointer: a sharded caller uploads
                                          * camera frames and hands the records straight to an RCCL all-gather (sharding.py) */

typedef struct opd_config {
    int32_t struct_size; /* = sizeof(opd_config), for forward compatibility */
    int32_t max_batch;   /* workspace is sized for max_batch frames of max_height x max_width pixels, in either orientation:   */
    int32_t max_height;  /* a call may pass any H x W with H, W <= max(max_height, max_width) and H * W <= max_height * max_width */
    int32_t max_width;   /* (the HF size rule maps a portrait camera frame to about 1333 x 750)                                    */
    int32_t flags;       /* OPD_FLAG_* */
    int32_t reserved[3];
} opd_config;

#define OPD_FLAG_NO_GRAPH 1 /* launch kernels eagerly instead of replaying a captured hipGraph */
#define OPD_FLAG_BF16 4 /* bf16 instead of fp16 as the 16-bit operand type of every activation buffer and GEMM weight (the type BASELINE.json
                         * configs[1] names; same MFMA rate on gfx950, 8 mantissa bits instead of 11: the boxes drift more, see DESIGN.md
                         * section 3).  The decoder's linear layers keep their split fp16 operands (fp32-grade) in both modes. */
#define OPD_FLAG_MULTI_STREAM 2 /* this handle is one of several that keep batches in flight on one GPU: kernel choices are made for
                                 * throughput (a launch's last, partly filled round overlaps other handles' work) rather than for latency */

/* One detection record (32 bytes).  Boxes are (x1,y1,x2,y2) in pixels of the ORIGINAL frame, as produced by
 * HF `post_process_object_detection` (HF:models/detr/image_processing_detr.py:805-856). */
typedef struct opd_det {
    float x1, y1, x2, y2;
    float score;
    int32_t label;       /* argmax over the first C classes ("no object" excluded) */
    int32_t query_index; /* decoder query that produced it (`Detection.query_index`, src/models/data_models.py:38) */
    int32_t frame;       /* index of the frame inside the batch */
} opd_det;

/* Architecture facts read back from a loaded model. */
typedef struct opd_model_info {
    int32_t depths[4];
    int32_t d_model, heads, ffn_dim, encoder_layers, decoder_layers, num_queries, num_classes_plus1;
    int32_t max_batch, max_height, max_width;
    int32_t device_ordinal;
    int64_t weight_bytes_device;
    int64_t workspace_bytes_device;
} opd_model_info;

/* Replaces `ViTDetector.__init__` + `load_model()` (deleted vit_detector.py 36-44, 81-99; same contract as
 * `YOLOv8Detector.load_model`, yolov8_detector.py:70-88): parse a safetensors checkpoint carrying the HF
 * `DetrForObjectDetection` state dict (5.x or 4.x key names), fold every FrozenBN into its convolution in fp32
 * (HF:models/detr/modeling_detr.py:179-215), convert to the device layouts and upload to GPU `device_ordinal`. */
OPD_API int opd_detr_create(const opd_config* cfg, const char* weights_path, int device_ordinal, opd_detr** out);

/* Replaces `cleanup_resources` / detector release (`src/utils/memory_utils.py:33-41`). */
OPD_API void opd_detr_destroy(opd_detr* m);

/* A second handle on the SAME model: own stream, workspace and graph cache, the weights in HBM shared with `src` (read-only after
 * creation; freed when the last handle that uses them is destroyed, in any order).  For several batches in flight on one GPU
 * (`HipDetrDetector(streams=N)`, bench.py): no second parse of the checkpoint, one copy of the 83 MB of weights for L2 and the
 * Infinity Cache to hold instead of N.  No reference counterpart (one detector object per process there). */
OPD_API int opd_detr_clone(const opd_detr* src, opd_detr** out);

OPD_API int opd_detr_info(const opd_detr* m, opd_model_info* info);

/* Replaces `with torch.no_grad(): outputs = model(pixel_values, pixel_mask)` in `ViTDetector.detect_batch`
 * (deleted vit_detector.py 508-550; HF:models/detr/modeling_detr.py:1329-1443), including the BGR->RGB / 1/255 /
 * ImageNet mean-std step of `_preprocess_batch` (562-578) when `pixel_format == OPD_PIXELS_U8_BGR_HWC`.
 * All B frames share one size HxW (pixel_mask all ones).  `enc_features` may be NULL.
 * `mem_kind` says whether pixels AND outputs are host or device pointers.  Synchronous: results are complete on
 * return. */
OPD_API int opd_detr_forward(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W,
                     float* logits, float* boxes, float* enc_features);

/* The same call for a RAGGED batch: `model(pixel_values, pixel_mask)` with a padding mask, i.e. what HF's
 * `DetrImageProcessor.pad` + the mask paths of the model do when the frames of a batch differ in size
 * (HF:models/detr/image_processing_detr.py:639-668 zero-pad after normalisation + pixel_mask;
 * HF:models/detr/modeling_detr.py:283-289 nearest down-sampling of the mask, 294-368 position embedding from the mask's
 * cumulative sums, 402-427 additive key mask in encoder self-attention and decoder cross-attention).
 * `pixels` is the H x W canvas batch with every frame in its top-left corner; `valid_hw` = host [B][2] int32 (height, width)
 * of each frame inside the canvas (NULL or all (H, W): identical to opd_detr_forward).  Canvas pixels outside a frame are
 * ignored (written as zeros on the device).  `enc_features` covers the whole canvas map, padded positions included. */
OPD_API int opd_detr_forward_ragged(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W,
                            const int32_t* valid_hw, float* logits, float* boxes, float* enc_features);

/* Device-side resize: frames at CAMERA resolution in, the resize half of `_preprocess_batch` on the GPU.
 * `frames` = [B][h][w][3] uint8 BGR (host or device per `mem_kind`), all of one size; they are resized to H x W — the caller
 * computes (H, W) with the HF size rule (HF:image_transforms.py:206-242; `model_input_size` in the Python shim) — by a kernel
 * that is BIT-EXACT with Pillow's 8-bit bilinear resampler, i.e. with `DetrImageProcessor.resize`
 * (HF:models/detr/image_processing_detr.py:424-436), then run through the same path as opd_detr_forward.
 * Outputs follow `mem_kind`. */
OPD_API int opd_detr_forward_resized(opd_detr* m, const uint8_t* frames, int mem_kind, int B, int h, int w, int H, int W,
                             float* logits, float* boxes, float* enc_features);
/* The resize alone (host in, host out): [B][h][w][3] -> [B][out_h][out_w][3]; for parity tests against Pillow. */
OPD_API int opd_detr_resize_u8(opd_detr* m, const uint8_t* frames, int B, int h, int w, int out_h, int out_w, uint8_t* out);

/* Replaces `_postprocess_batch` part 1 = HF `post_process_object_detection` (deleted vit_detector.py 591-647;
 * HF:models/detr/image_processing_detr.py:805-856): softmax over C+1, max over the first C classes, cxcywh->xyxy,
 * scale by the ORIGINAL (height,width) of each frame, keep score > threshold.  Runs on the device on the logits and
 * boxes of the LAST forward of this handle.  `orig_hw` = [B][2] int32 host array (height, width) or NULL (= model
 * input size).  `out` (host) receives `counts[b]` records for frame b at out[b*Q ...]; records keep query order. */
OPD_API int opd_detr_postprocess(opd_detr* m, float threshold, const int32_t* orig_hw, opd_det* out, int32_t* counts);

/* One call = forward + device post-process, pixels in HBM when `mem_kind == OPD_MEM_DEVICE` (the benchmark's
 * timed region).  Equivalent to opd_detr_forward(..., NULL, NULL, NULL) followed by opd_detr_postprocess(...). */
OPD_API int opd_detr_detect(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W,
                    float threshold, const int32_t* orig_hw, opd_det* out, int32_t* counts);
/* With `mem_kind == OPD_MEM_DEVICE`, `out` ([B][Q] records) and `counts` ([B]) are DEVICE pointers too, so a sharded
 * caller can hand them straight to an RCCL all-gather; `orig_hw` is always a host array. */
/* Asynchronous submission for throughput-oriented callers: enqueues the forward and the post-process on the handle's stream
 * and returns with a `ticket` (0..3; at most 4 submissions may be outstanding per handle: a fifth returns OPD_ESTATE until the
 * oldest ticket has been waited for, and waiting twice for one ticket is OPD_ESTATE too); `out` / `counts` of a submission
 * are complete after opd_detr_wait(m, ticket) (`mem_kind` as in opd_detr_detect: host pixels are staged with an asynchronous
 * copy, host outputs travel through pinned memory and are delivered by opd_detr_wait; `pixels`, `out` and `counts` must stay
 * valid and untouched until that wait returns).  Work of consecutive submissions to ONE
 * handle runs in submission order; SEVERAL handles on one device (own stream, workspace and captured graph each) overlap:
 * the latency-bound tail of one batch fills the CUs the next batch's trunk leaves idle (+25 % frames/s with three handles at
 * batch 8). */
OPD_API int opd_detr_detect_async(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W, float threshold,
                          const int32_t* orig_hw, opd_det* out, int32_t* counts, int* ticket);
OPD_API int opd_detr_wait(opd_detr* m, int ticket);
/* Camera-resolution form (see opd_detr_forward_resized): resize on the device, detect, and scale the boxes back to the
 * camera frame size (h, w). */
OPD_API int opd_detr_detect_resized(opd_detr* m, const uint8_t* frames, int mem_kind, int B, int h, int w, int H, int W,
                            float threshold, opd_det* out, int32_t* counts);
/* The same for a LIST of host frames, one pointer per frame (what the reference hands a detector: detect_batch(frames: List[np.ndarray]),
 * deleted vit_detector.py:508; DetectorPort.detect(frames: Sequence[FrameDTO]), src/core/interfaces.py:30-34): frames[b] = [h][w][3] uint8
 * BGR, all of one size, each uploaded from where it lies -- no stacked copy of the batch on the host (25.6 MB at batch 8: 0.75 ms of a
 * 3.4-ms step).  (h, w) == (H, W): no resize.  mem_kind: OPD_MEM_HOST or OPD_MEM_HOST_PIXELS_DEVICE_OUT (the frames are host memory). */
OPD_API int opd_detr_detect_frames(opd_detr* m, const uint8_t* const* frames, int mem_kind, int B, int h, int w, int H, int W,
                                   float threshold, opd_det* out, int32_t* counts);
/* `detect_with_features(frame)` in ONE call (yolov8_detector.py:134-159: detect, then pool the encoder map under every detection's box,
 * src/tracking/feature_extractor.py:39-88): opd_detr_detect_frames on host frames + the appearance feature of every record of class `label`
 * (ROI mean-pool + L2 norm exactly as opd_detr_roi_features computes it for the record's box), pooled while the records are still on the
 * device -- one host wait instead of two.  features: [B][num_queries][d_model] fp32 (host), row = the record's query_index; rows of queries
 * without a record of that class are NOT written (whatever the buffer held).  Suppression: by default (opd_detr_set_nms off) it happens
 * afterwards on the host (opd_person_nms), and a suppressed record's row is simply unused; with opd_detr_set_nms on, the records are
 * suppressed on the device BEFORE the pooling, come back final in score order, and rows are written for kept records only. */
OPD_API int opd_detr_detect_frames_features(opd_detr* m, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold,
                                            int label, opd_det* out, int32_t* counts, float* features);
/* The same call with the reference's DEFAULT appearance feature instead (`YOLOv8Detector.extract_features`, yolov8_detector.py:161-190, which
 * `detect_with_features` calls: crop every detection, `FeatureExtractor.extract_batch`): the colour histogram of opd_color_features for every
 * record of class `label`, computed from the CAMERA-resolution frames this call has just uploaded (h x w, at most 4096 x 4096) under the
 * record's box (x1, y1, float32(x2 - x1), float32(y2 - y1)) -- the float32 (x, y, w, h) the Python shim passes on for a `Detection.bbox` --
 * so a row is bit-identical to opd_color_features on that box.  features: [B][num_queries][256] fp32 (host), row = the record's
 * query_index; rows of queries without a record of that class are NOT written.  Needs d_model = 256 (the handle's feature area). */
OPD_API int opd_detr_detect_frames_color(opd_detr* m, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold,
                                         int label, opd_det* out, int32_t* counts, float* features);
/* Ragged-batch form (see opd_detr_forward_ragged); `valid_hw` and `orig_hw` are host arrays. */
OPD_API int opd_detr_detect_ragged(opd_detr* m, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W,
                           const int32_t* valid_hw, float threshold, const int32_t* orig_hw, opd_det* out, int32_t* counts);

/* Replaces `_postprocess_batch` part 2 (deleted vit_detector.py 591-647; `docs/plan.md:30`,
 * `config.yaml.disabled:38`): keep `label == person_label` (pass -1 to keep every class), greedy IoU-NMS in
 * descending score order at `nms_threshold` (pass >= 1 to disable).  Host-side, in place: compacts `dets[0..n)` and
 * returns the new count (>= 0) or a negative error. */
OPD_API int opd_person_nms(opd_det* dets, int n, int person_label, float nms_threshold);
/* The same for a whole batch in one call: frame f owns `dets[f * stride .. f * stride + counts[f])` (the fixed-slot layout
 * opd_detr_detect writes, stride = num_queries); every frame is compacted in place and `counts[f]` becomes its new count.
 * A negative `counts[f]` (padding slot of an uneven shard) is left alone.  Returns 0 or a negative error. */
OPD_API int opd_person_nms_batch(opd_det* dets, int32_t* counts, int n_frames, int stride, int person_label, float nms_threshold);
/* The same filter and suppression ON THE DEVICE, inside every call that delivers records.  Handle state; a negative `nms_threshold`
 * turns it off, the state after opd_detr_create and opd_detr_clone.  While on, every entry point that delivers records (blocking,
 * opd_detr_detect_async / opd_detr_wait, _resized, _ragged, _frames, _frames_features, _frames_color, _frames_floor, _frames_reid,
 * opd_detr_postprocess, opd_comm_detect), from the next submission on, runs one more kernel directly behind the post-process, in place
 * on whichever buffers it wrote (the handle's, or the caller's device pointers), before the feature, floor and Re-ID stages: the
 * records come back FINAL, per frame in descending score order (ties in query order), exactly what opd_person_nms_batch(person_label,
 * nms_threshold) makes of the unsuppressed records -- so host suppression applied again changes nothing.  `person_label` < 0 keeps
 * every class; `nms_threshold` >= 1 filters and sorts without suppressing.  The forward graph is not recaptured.  OPD_EINVAL: a null
 * handle, a NaN threshold. */
OPD_API int opd_detr_set_nms(opd_detr* m, int person_label, float nms_threshold);
/* opd_person_nms_batch for DEVICE-resident records (the gathered buffer of a sharded step, the outputs of a DEVICE_OUT call): `dets`
 * [n_frames][stride] and `counts` [n_frames] are device-accessible memory on `m`'s device, rewritten in place on `m`'s stream; the call
 * returns when they are final.  A negative count is left alone.  OPD_EINVAL before any device work: a null handle, n_frames < 0,
 * stride < 1 or > 128, pointers that are not device-accessible memory.  OPD_EINVAL after the wait: a count above the stride (that
 * frame's records and count are left as they were; the other frames are done). */
OPD_API int opd_detr_nms_records(opd_detr* m, opd_det* dets, int32_t* counts, int n_frames, int stride, int person_label, float nms_threshold);

/* ---- tiled detection: a frame cut into overlapping tiles of ONE size, detected and merged across the seams in one call ------------
 * One merged detection (48 bytes), in pixels of the FRAME: what `tiling.merge_tile_detections` returns as `bbox` (x, y, w, h in
 * float64), with the score, label and `query_index` of the per-tile record that opened it and the index of that record's tile. */
typedef struct opd_tile_det { double x, y, w, h; float score; int32_t label, query_index, tile; } opd_tile_det;
/* `struct_size` = sizeof of this struct (40).  `person_label` / `tile_nms_threshold`: the per-tile filter and suppression, as in
 * opd_detr_set_nms (a threshold >= 1 filters and sorts only).  The merge (float64, the Python rule operation for operation): in
 * descending score order a record is dropped when its IoU with a kept box exceeds `merge_nms_threshold` (>= 1: nothing is ever
 * absorbed), and when it comes from another tile than the kept box, one of the two has a side within `edge_tolerance` x tile size of
 * an INTERIOR tile edge and their intersection covers more than `merge_threshold` of the smaller, the kept box grows to their union. */
typedef struct opd_tile_params { int32_t struct_size, person_label; float tile_nms_threshold; float pad;
                                 double merge_nms_threshold, merge_threshold, edge_tolerance; } opd_tile_params;
/* `frames`: n_frames HOST pointers, each a contiguous uint8 [h][w][3] BGR frame.  `tiles_yxhw`: [n_tiles][4] = (y0, x0, th, tw), the
 * same windows for every frame.  Each frame is uploaded ONCE; its tiles are resampled to H x W from where it lies on the device
 * (Pillow-exact, byte for byte opd_detr_resize_u8 of contiguous copies of the windows), go through one forward of n_frames x n_tiles
 * images, are post-processed to tile pixels, filtered and suppressed per tile and merged per frame, all on the device behind ONE wait.
 * `out`: [n_frames][n_tiles x num_queries] records, `counts`: [n_frames], host memory; frame f's records are out[f x n_tiles x
 * num_queries ...), in the order the Python rule keeps them.  The handle's opd_detr_set_nms state is neither used nor changed.
 * OPD_EINVAL before any device call: a null pointer, a wrong struct_size, a NaN or negative tile_nms_threshold,
 * n_frames x n_tiles outside [1, max_batch], a window outside the frame, windows of MORE THAN ONE SIZE (one forward has one model
 * size), n_tiles x num_queries > 1024 candidates per frame, H x W outside the handle's maximum. */
OPD_API int opd_detr_detect_tiled(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w,
                                  const int32_t* tiles_yxhw, int n_tiles, int H, int W, float threshold,
                                  const opd_tile_params* p, opd_tile_det* out, int32_t* counts);
/* The merge alone, on records of the caller (the gathered buffer of a sharded tiled step): HOST `recs` [n_frames x n_tiles][stride] in
 * tile pixels and `tile_counts` [n_frames x n_tiles], taken as they are (no filter, no suppression: `person_label` and
 * `tile_nms_threshold` are not read); the windows may differ in size.  Blocking; `out` [n_frames][n_tiles x stride], `counts`
 * [n_frames].  A negative tile count counts as 0.  OPD_EINVAL before any device call: a null pointer, a wrong struct_size, n_frames < 0,
 * n_tiles < 1, stride < 1, n_tiles x stride > 1024, a window outside the h x w frame.  OPD_EINVAL after the wait: a tile count above
 * the stride (that frame comes back with count 0; the other frames are done). */
OPD_API int opd_detr_merge_tiles(opd_detr* m, const opd_det* recs, const int32_t* tile_counts, int n_frames, int n_tiles, int stride,
                                 const int32_t* tiles_yxhw, int h, int w, const opd_tile_params* p, opd_tile_det* out, int32_t* counts);

/* Page-locked host memory for frame batches handed over with OPD_MEM_HOST: the upload of such a buffer is one asynchronous DMA
 * instead of the runtime's staged copy of pageable memory.  Optional (any host pointer is accepted everywhere); the Python shim
 * stacks the caller's frames (`detect_batch(frames: list[np.ndarray])`, the reference's calling convention) directly into it. */
OPD_API int opd_host_alloc(size_t bytes, void** out);
OPD_API void opd_host_free(void* p);

/* "Next" row: replaces `SimilarityCalculator.compute_similarity_matrix` / `compute_distance_matrix`
 * (`src/tracking/similarity.py:42-220`), the tracker's cost matrix built right after the detect path:
 * similarity[i][j] = clip((aw * clip(f1_i . f2_j, -1, 1) + mw * IoU(box1_i, box2_j)) / (weights used), 0, 1); a row without
 * features (has == 0, or a NULL feature matrix) drops the appearance term and renormalises.  Boxes are (x, y, w, h).
 * All pointers are host pointers; `out` = [n1][n2] f32; `as_distance` != 0 returns 1 - similarity.  Runs on the device
 * `device_ordinal`; needs no model handle. */
OPD_API int opd_similarity_matrix(int device_ordinal, const float* feats1, const float* boxes1, const uint8_t* has1, int n1,
                          const float* feats2, const float* boxes2, const uint8_t* has2, int n2, int D,
                          double appearance_weight, double motion_weight, int as_distance, float* out);

/* Replaces `FeatureExtractor.extract_roi_features` on the DETR encoder map
 * (`src/tracking/feature_extractor.py:39-88`; deleted vit_detector.py 224-273): for each (x,y,w,h) box in original
 * pixels, mean-pool the last forward's encoder map of frame `frame` over the int-truncated, clamped ROI and
 * L2-normalise (x / (||x|| + 1e-8)).  `features` = host [n][D] f32.  Runs on the device. */
OPD_API int opd_detr_roi_features(opd_detr* m, int frame, const float* boxes_xywh, int n, int orig_h, int orig_w,
                          float* features);

/* Replaces `FeatureExtractor.extract_batch` on the crops `YOLOv8Detector.extract_features` cuts (src/tracking/feature_extractor.py:90-137,
 * src/detection/yolov8_detector.py:176-185), the tracker's appearance feature whenever `tracking.reid.enabled` is false (the default).
 * Box i = (x, y, w, h) float32 in pixels of frame box_frame[i] (host int32; NULL = frame 0); frames[f] = [h][w][3] uint8 BGR with
 * (h, w) = frame_hw[2f], frame_hw[2f + 1] (host int32), at most 4096 x 4096.  The crop is x1 = int(max(0, x)), x2 = int(min(W, x + w)),
 * same for y; x2 <= x1 or y2 <= y1 takes the reference's 64 x 32 zero image.  Row = 64 bin counts (bin = value >> 2) of B, of G, of R,
 * then mean, std of B, of G, of R (population std), zeros up to 256, the whole row divided by (its L2 norm + 1e-8).  Counts and sums are
 * integers on the device and the statistics and the norm are fp64, so a row depends on its pixels alone (not on the other boxes, the
 * launch shape or mem_kind) and lies within 2^-24 of the exactly evaluated formula.  OPD_MEM_DEVICE: frames are device pointers, read in
 * place.  OPD_MEM_HOST: one transfer of the crops' source windows, or of the named frames whole when that is fewer bytes; one host wait.
 * `out` = host float32 [n_boxes][256].  n_boxes == 0 is OPD_OK.  Runs on device `device_ordinal`; needs no model handle. */
OPD_API int opd_color_features(int device_ordinal, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind,
                               const float* boxes_xywh, const int32_t* box_frame, int n_boxes, float* out);

/* Replaces `get_attention_map` / `_extract_attention_map` (deleted vit_detector.py 392-446, `coverage.json:1`; the surviving stand-in
 * returns None, `src/detection/yolov8_detector.py:243-254`; consumer: `Visualizer.draw_attention_map`, `src/visualization/visualizer.py:148-200`,
 * which takes a 1-D or 2-D array in [0, 1]).  The DETR-era source is gone, so the definition is this build's: the decoder's
 * cross-attention weights of layer `layer` (negative: counted from the last) of the LAST forward's frame `frame`, averaged over the
 * heads and over the `n_queries` query indices in `queries` (n_queries == 0: all queries).  `out` = host [fh * fw] f32, row-major over
 * the feature map of that forward (fh = ceil(H/32), fw = ceil(W/32)), summing to 1; `out_capacity` = floats the caller allocated: a
 * map larger than that is OPD_EINVAL, nothing is written.  Runs on the device from the q / k operands the forward left there, so the
 * call belongs to the caller that ran that forward: no other submission to this handle in between (single caller per handle). */
OPD_API int opd_detr_attention_map(opd_detr* m, int frame, int layer, const int32_t* queries, int n_queries, float* out, int out_capacity);

/* ---- multi-GPU: the path's one exchange step ------------------------------------------------------------------------------
 * The reference has no distributed mode; the port it reserves for batched detectors is `DetectorPort.detect(frames: Sequence[FrameDTO])`
 * (`src/core/interfaces.py:30-34`, home `src/adapters/__init__.py:1`).  Frames are independent, so the path shards by frame: one process
 * per GPU, each with its own detector handle, and ONE RCCL all-gather of fixed-size records per exchange (opd_det x num_queries per frame
 * slot + one int32 count per slot; count -1 = the slot holds no frame).  An `opd_comm` is a LANE: one detector handle's send / receive
 * buffers and events on a communicator that all lanes of the rank share (opd_comm_create makes the communicator and its first lane,
 * opd_comm_attach further lanes for further handles).  A step: forward -> post-process (writes the lane's send buffer) on the HANDLE's stream;
 * ncclAllGather -> copy to page-locked host memory on the COMMUNICATOR's own stream, which waits for the handle's stream through an event;
 * one host wait (opd_comm_wait).  All all-gathers of a rank are enqueued on that one stream in the order opd_comm_exchange was called: every
 * rank must call it in the same order across its lanes.  RCCL is resolved at run time (librccl.so.1); single-GPU callers never load it.
 * The 128-byte unique id travels from rank 0 to the other ranks by whatever launched them (file, socket, MPI, a torch.distributed store):
 * the library does no rendezvous.  ncclCommInitRank blocks until every rank has arrived: callers check opd_comm_available() on every rank
 * and agree on it first, and bound the set-up with a watchdog of their own (sharding.py, bench.py). */
typedef struct opd_comm opd_comm;
#define OPD_COMM_ID_BYTES 128
OPD_API int opd_comm_available(void);          /* OPD_OK when librccl could be resolved in this process: every rank checks BEFORE any rank enters the collective set-up */
OPD_API int opd_comm_unique_id(void* id128);   /* rank 0 only: ncclGetUniqueId */
/* collective over the `world` ranks (ncclCommInitRank): every rank passes the same id, its rank, and its OWN handle (device and stream) */
OPD_API int opd_comm_create(const void* id128, int rank, int world, opd_detr* m, opd_comm** out);
/* A further LANE on `parent`'s communicator for another detector handle of the same device (a rank that keeps several batches in flight):
 * own send / receive buffers and events, the SAME RCCL communicator.  All all-gathers of a rank are enqueued on the communicator's own
 * stream in the order opd_comm_exchange was called, so every rank must call it in the same order across its lanes.  Local, not collective. */
OPD_API int opd_comm_attach(opd_comm* parent, opd_detr* m, opd_comm** out);
/* Lanes may be destroyed in any order; the communicator goes with the last one.  Destroying the detector handle first is allowed: its lanes
 * then return OPD_ESTATE from every call and only opd_comm_destroy remains valid on them. */
OPD_API void opd_comm_destroy(opd_comm* c);
OPD_API int opd_comm_info(const opd_comm* c, int* rank, int* world);
/* A lane holds up to TWO exchanges: while one travels (issued, not yet waited for) the next may be begun, filled and issued; opd_comm_wait
 * delivers them oldest first; a third opd_comm_begin returns OPD_ESTATE.
 * One exchange = begin(slots) ; detect(slot0, frames ...) once or several times (a shard larger than max_batch goes in chunks) ; exchange ;
 * wait.  `slots` = frame slots per rank, the same number on every rank (an uneven shard leaves trailing slots at count -1).
 * opd_comm_detect = opd_detr_detect_async into the send buffer at slot0 (arguments as there); nothing synchronises before opd_comm_wait,
 * which delivers every rank's records: out_all [world][slots][num_queries], counts_all [world][slots] (host). */
OPD_API int opd_comm_begin(opd_comm* c, int slots);
OPD_API int opd_comm_detect(opd_comm* c, int slot0, const void* pixels, int pixel_format, int mem_kind, int B, int H, int W, float threshold,
                            const int32_t* orig_hw);
/* Device pointers of slot `slot0` of the send buffer (records [.][num_queries], counts [.]): for callers that fill the slots through another
 * entry point with device outputs (opd_detr_detect_resized / _ragged with OPD_MEM_HOST_PIXELS_DEVICE_OUT) on the SAME handle. */
OPD_API int opd_comm_buffers(opd_comm* c, int slot0, void** records, void** counts);
OPD_API int opd_comm_exchange(opd_comm* c);
OPD_API int opd_comm_wait(opd_comm* c, opd_det* out_all, int32_t* counts_all);

/* Device time (ms) of the last DETECT call (opd_detr_detect and its variants: forward + post-process) per stage, measured with HIP events on the handle's stream:
 * [0] preprocess+stem+pool, [1] stage1, [2] stage2, [3] stage3, [4] stage4, [5] projection+encoder, [6] decoder+heads,
 * [7] post-process.  Only filled when profiling is on: opd_detr_set_profiling(m, 1) = the forward is launched EAGERLY with an event pair
 * around every launch (opd_detr_kernel_times; the eager launches and their events add ~10 us per launch to the stage times), (m, 2) =
 * the stage marks are recorded INSIDE the replayed hipGraph: the stage times of the path as a caller gets it (no per-kernel times). */
OPD_API int opd_detr_set_profiling(opd_detr* m, int enabled);
OPD_API int opd_detr_stage_times(const opd_detr* m, float* ms8);
/* Per-kernel-class totals of the last profiled forward, from HIP event pairs recorded around EVERY launch on the
 * handle's stream: class 0 = conv_gemm_kernel on backbone convolutions (+ input projection), 1 = conv_gemm_kernel as
 * transformer linear layer, 2 = attention_kernel, 3 = reserved.  ms4[c] = summed device time, launches4[c] = number of
 * launches, flops4[c] = summed ALGORITHMIC FLOPs (2 x MAC) of those launches. */
OPD_API int opd_detr_kernel_times(const opd_detr* m, float* ms4, int32_t* launches4, double* flops4);
/* The same event pairs by KERNEL: one row per kernel instantiation of the last profiled forward (mode 1), longest first -- `name` as rocprofv3
 * prints it minus namespace and signature (e.g. "btail256_kernel<256, false>"), so a row can be checked against a kernel-trace summary;
 * launches, summed device time (ms) and summed algorithmic FLOPs (0 for launches that are not GEMM-shaped).  *count = rows available;
 * at most `capacity` are written. */
typedef struct opd_kernel_stat { char name[96]; int32_t launches; float ms; double flops; } opd_kernel_stat;
OPD_API int opd_detr_kernel_table(const opd_detr* m, opd_kernel_stat* out, int capacity, int* count);

/* ---- Re-ID features: the CLIP ViT image tower or OSNet (second handle type, own weights, workspace, stream and graphs) ---------------
 * One handle type serves the reference's two `ReIDFeatureExtractor` models (src/tracking/reid_feature_extractor.py:369-463), chosen by
 * opd_reid_config.model.  Per box, both crop the frame at x1 = int(max(0, x)), x2 = int(min(W, x + w)) (same for y), BGR -> RGB, and
 * return float32 [n_boxes][feature_dim] rows of unit L2 norm.
 *  - OPD_REID_MODEL_CLIP replaces `CLIPReIDExtractor.extract_features` (lines 108-153): an empty crop becomes a 224 x 224 zero image;
 *    CLIPImageProcessor (Pillow bicubic resize to shortest edge 224, centre crop 224, /255, CLIP mean / std), then
 *    `CLIPModel.get_image_features`.
 *  - OPD_REID_MODEL_OSNET replaces `OSNetReIDExtractor.extract_features` (lines 295-350): an empty crop becomes a 256 x 128 zero image;
 *    Pillow bilinear resize to 256 x 128 (no aspect ratio kept, no centre crop), ToTensor, ImageNet mean / std, then torchreid's
 *    `osnet_x1_0` in eval mode without its classifier (512 features after fc + BatchNorm1d + ReLU). */
typedef struct opd_reid opd_reid; /* opaque Re-ID handle */

#define OPD_REID_MODEL_CLIP 0  /* HF CLIP vision tower (a zeroed config means CLIP) */
#define OPD_REID_MODEL_OSNET 1 /* torchreid OSNet */

typedef struct opd_reid_config {
    int32_t struct_size; /* = sizeof(opd_reid_config) */
    int32_t max_crops;   /* workspace and launch plans are sized for this many crops; a call with more boxes runs in chunks */
    int32_t flags;       /* OPD_FLAG_NO_GRAPH: eager launches instead of one captured hipGraph per crop-count bucket */
    int32_t model;       /* OPD_REID_MODEL_CLIP or OPD_REID_MODEL_OSNET; any other value is OPD_EINVAL */
    int32_t reserved[4];
} opd_reid_config;

/* CLIP fills every field.  OSNet fills feature_dim (512), hidden (the last stage width, 512 for x1.0), max_crops, device_ordinal, model
 * and the two byte counts; tokens, layers, heads, mlp_dim and patch are 0. */
typedef struct opd_reid_model_info {
    int32_t feature_dim, tokens, hidden, layers, heads, mlp_dim, patch, max_crops;
    int32_t device_ordinal, model;
    int64_t weight_bytes_device;
    int64_t workspace_bytes_device;
} opd_reid_model_info;

/* Parse a safetensors file holding an HF `CLIPModel` or `CLIPVisionModelWithProjection` state dict (`vision_model.*` and
 * `visual_projection.weight`; `text_model.*` is ignored), infer the architecture from the shapes (head_dim 64, or
 * `num_attention_heads` of a config.json beside the file) and upload it.  The schema is checked before the device is touched:
 * head_dim != 64, more than 64 tokens, a hidden size that is not a multiple of 128 (or above 1024), or an image size other than 224
 * return OPD_ESCHEMA with a message naming the limit.
 * OPD_REID_MODEL_OSNET: a safetensors file holding torchreid's OSNet state dict under its own key names (`conv1.conv.weight`,
 * `conv2.0.conv2b.1.bn.running_var`, `fc.1.weight`, ...; `classifier.*` and integer tensors such as `num_batches_tracked` are ignored).
 * The four stage widths and the blocks per stage are inferred from the shapes; BatchNorm is folded into the convolutions and into fc in
 * fp32 at load.  OPD_ESCHEMA (checked before the device is touched) names a missing tensor, a tensor of the wrong shape, an
 * instance-norm variant (osnet_ain / osnet_ibn: a `bn` without running statistics, or `IN` tensors), an fc width other than 512, or a
 * width the kernels cannot run: the stem width must be a multiple of 16 up to 64 and every stage width a multiple of 64 (the last one
 * up to 512).  osnet_x1_0 (64, 256, 384, 512) and osnet_x0_5 (32, 128, 192, 256) run; osnet_x0_75 (stage width 288) and osnet_x0_25
 * (stage widths 64, 96 with stem 16: 96 is refused) do not. */
OPD_API int opd_reid_create(const opd_reid_config* cfg, const char* weights_path, int device_ordinal, opd_reid** out);
OPD_API void opd_reid_destroy(opd_reid* r);
OPD_API int opd_reid_info(const opd_reid* r, opd_reid_model_info* info);
/* Features of `n_boxes` boxes (x, y, w, h in frame pixels, host [n_boxes][4]) on `n_frames` frames: box i lies on frame box_frame[i]
 * (host int32; NULL = frame 0).  frames[f] = [h][w][3] uint8 BGR with (h, w) = frame_hw[2f], frame_hw[2f + 1] (host int32); host memory
 * for OPD_MEM_HOST (only each crop's source window is copied to the device, packed into one transfer), device pointers read in place
 * for OPD_MEM_DEVICE.  `out` = host float32 [n_boxes][feature_dim].  Synchronous. */
OPD_API int opd_reid_extract(opd_reid* r, const uint8_t* const* frames, const int32_t* frame_hw, int n_frames, int mem_kind,
                             const float* boxes_xywh, const int32_t* box_frame, int n_boxes, float* out);
/* opd_detr_detect_frames (host frames, host outputs) plus the Re-ID feature row of the first `slots` records labelled `label`, taken in
 * (frame, record index) order, behind ONE host wait: the crops are planned on the device from the records (box = x1, y1,
 * float32(x2 - x1), float32(y2 - y1), as opd_reid_extract would be handed it) and read in place from the camera-resolution frames this
 * call uploaded.  `features` = host float32 [slots][feature_dim]; row k belongs to record slot_map[k] = frame * num_queries +
 * query_index (host int32 [slots]); *n_person = the number of such records in the batch.  Rows and slot_map entries k >= min(*n_person,
 * slots) are not written.  *n_person > slots is not an error: the caller fetches the remaining rows with opd_reid_extract.  Suppression:
 * by default (opd_detr_set_nms off) it stays on the host afterwards (opd_person_nms), the slots go to records in query order and a
 * suppressed record's row is unused; with opd_detr_set_nms on, the records are suppressed on the device first, *n_person counts the
 * KEPT records, and the slots go to the kept records of each frame in score order.  OPD_EINVAL before any device work: a null
 * handle or output, slots < 1 or > max_crops, handles on different devices, B > max_batch, frame sizes outside the detector handle's
 * limits.
 * A Re-ID handle serves ONE call at a time: a thread that enters this call or opd_reid_extract while another call on the same opd_reid
 * is running waits for it to finish. */
OPD_API int opd_detr_detect_frames_reid(opd_detr* m, opd_reid* r, const uint8_t* const* frames, int B, int h, int w, int H, int W,
                                        float threshold, int label, int slots, opd_det* out, int32_t* counts,
                                        float* features /*[slots][feature_dim]*/, int32_t* slot_map /*[slots]*/, int32_t* n_person);

/* ---- Sparse optical flow: pyramidal Lucas-Kanade between consecutive frames (third handle type: two gray pyramids, own stream) --------
 * Replaces the per-frame work of `OpticalFlowTracker.track` (src/tracking/lightweight_tracker.py:141-202), which the reference's hybrid
 * tracker runs on every frame its detector skips: cv2.cvtColor(BGR2GRAY) and cv2.calcOpticalFlowPyrLK(prev_gray, gray, points, winSize,
 * maxLevel, criteria).  The arithmetic is OpenCV's (gray weights, 5 x 5 pyramid filter, Scharr derivatives, the same range, eigenvalue
 * and stopping tests) with the window interpolation and sums in float32 where OpenCV uses 14-bit fixed point.  Nothing
 * here is compared against cv2: the kernels are pinned to a float64 restatement of this arithmetic and to analytically known
 * displacements. */
typedef struct opd_flow opd_flow; /* opaque flow handle */

typedef struct opd_flow_config {
    int max_h, max_w;        /* buffers are sized for frames up to max_h x max_w pixels (each up to 8192) */
    int max_points;          /* ... and up to this many points per call */
    int win;                 /* window edge, odd, 3 .. 21 (0 = 21: winSize (21, 21)) */
    int max_level;           /* pyramid levels above level 0, up to 7 (0 = 3; a level no larger than the window ends the pyramid) */
    int max_iter;            /* iterations per level (0 = 30) */
    float epsilon;           /* stop when the step is at most this long (0 = 0.01; negative = never by this test) */
    float min_eig_threshold; /* a point is lost when the smaller eigenvalue of its gradient matrix / win^2 is below this (0 = 1e-4) */
} opd_flow_config;

OPD_API int opd_flow_create(const opd_flow_config* cfg, int device_ordinal, opd_flow** out);
OPD_API void opd_flow_destroy(opd_flow* f);
/* The frame points will be tracked FROM (`prev_gray`): [h][w][3] uint8 BGR, host memory (OPD_MEM_HOST) or a device pointer read in
 * place (OPD_MEM_DEVICE), h <= max_h, w <= max_w.  Any earlier reference is dropped; the size may change here. */
OPD_API int opd_flow_set_reference(opd_flow* f, const uint8_t* bgr, int mem_kind, int h, int w);
/* Where the `n` points pts_xy [n][2] (x, y; host float32) of the reference frame lie in frame `bgr` (same size as the reference):
 * next_xy [n][2] and status [n] (1 = found, 0 = lost: outside the frame by more than the window, or no texture), both host memory.
 * Afterwards `bgr` is the reference (also when n = 0).  OPD_ESTATE before a reference was set.  Synchronous: one wait.  A device frame must be
 * complete before the call: the handle's stream is not ordered after the stream that wrote it. */
OPD_API int opd_flow_track(opd_flow* f, const uint8_t* bgr, int mem_kind, int h, int w, const float* pts_xy, int n, float* next_xy,
                           uint8_t* status);

/* ---- Floor map: camera pixels -> floor-map pixels / mm and zone membership (fourth handle type: an immutable model, own stream) ---------
 * The reference's Phase 3 per detection (`TransformPhase.execute`, src/pipeline/phases/transform.py:257-330): foot point of the box ->
 * optional lens undistortion (piecewise-affine and thin-plate-spline only) -> homography / piecewise affine / thin-plate spline ->
 * floor pixels, mm and the bounds test -> `ZoneClassifier.classify`.  All arithmetic is float64, one wave per record, without fused
 * multiply-adds: the operations of the numpy restatement in tests/floor_common.py, one for one.  A record's
 * result depends on its box and the model only.  Triangulation, the affine matrices and the spline coefficients come from the host
 * (floor.py: scipy / numpy, as the reference computes them); the device never triangulates. */
typedef struct opd_floor opd_floor; /* opaque floor-map handle */

#define OPD_FLOOR_HOMOGRAPHY 0
#define OPD_FLOOR_PWA 1
#define OPD_FLOOR_TPS 2
#define OPD_FLOOR_MAX_POINTS 256
#define OPD_FLOOR_MAX_TRIANGLES 512
#define OPD_FLOOR_MAX_ZONES 64
#define OPD_FLOOR_MAX_VERTICES 64 /* per polygon */
#define OPD_FLOOR_VALID 1u        /* opd_floor_rec.flags: always set (the reference's transformers never fail a point) */
#define OPD_FLOOR_WITHIN 2u       /* 0 <= px[0] < width_px && 0 <= px[1] < height_px */
#define OPD_FLOOR_EXTRAPOLATED 4u /* piecewise affine: no triangle holds the point, the one with the nearest centroid was used */

/* Everything is copied at creation.  Arrays a method does not use may be NULL. */
typedef struct opd_floor_config {
    int32_t method;               /* OPD_FLOOR_HOMOGRAPHY, OPD_FLOOR_PWA or OPD_FLOOR_TPS */
    int32_t n_points;             /* control points (PWA, TPS): 3 .. 256 */
    int32_t n_triangles;          /* PWA: 1 .. 512 */
    int32_t n_zones;              /* 0 .. 64 */
    int32_t has_distortion;       /* != 0: undistort with `intrinsics` and `distortion` first (ignored for the homography, as in the reference) */
    int32_t allow_overlap;        /* 0: keep only the zone with the smallest (priority or +inf, position in the list) */
    int32_t width_px, height_px;  /* floor map size, for the bounds test */
    double H[9];                  /* homography, row-major; |det| >= 1e-10 */
    double scale_x_mm_per_px, scale_y_mm_per_px;
    double intrinsics[4];         /* fx, fy, cx, cy */
    double distortion[5];         /* k1, k2, p1, p2, k3 (OpenCV's order) */
    double tps_affine[6];         /* TPS: a0, a1, a2 of x, then of y: a0 + a1 x + a2 y */
    const double* points;         /* [n_points][2] control points in camera pixels */
    const int32_t* triangles;     /* PWA: [n_triangles][3] indices into `points` (scipy.spatial.Delaunay.simplices) */
    const double* affine;         /* PWA: [n_triangles][6], rows x and y of the triangle's matrix: (a0 x + a1 y) + a2 */
    const double* tps_weights;    /* TPS: [n_points][2] (w_x, w_y) */
    const double* zone_vertices;  /* [zone_offsets[n_zones]][2] floor pixels, the polygons one behind the other */
    const int32_t* zone_offsets;  /* [n_zones + 1] first vertex of every polygon; 3 .. 64 vertices each */
    const double* zone_priority;  /* [n_zones]; NaN = the zone has none.  NULL = none has one */
} opd_floor_config;

typedef struct opd_floor_rec {
    double px[2];       /* floor-map pixels */
    double mm[2];       /* px * scale */
    uint64_t zone_mask; /* bit z: zone z holds px (after the allow_overlap rule) */
    int32_t triangle;   /* PWA: the triangle used; -1 for the other methods */
    uint32_t flags;     /* OPD_FLOOR_VALID | OPD_FLOOR_WITHIN | OPD_FLOOR_EXTRAPOLATED */
} opd_floor_rec;

typedef struct opd_floor_model_info {
    int32_t method, n_points, n_triangles, n_zones, n_edges, has_distortion, allow_overlap, device_ordinal;
} opd_floor_model_info;

/* OPD_EINVAL, before the device is touched, for: an unknown method, a count above the limits, fewer than 3 control points, a singular H
 * (|det| < 1e-10, the reference's test), a triangle index outside the points, a polygon of fewer than 3 or more than 64 vertices, a
 * missing array, a zero focal length with has_distortion. */
OPD_API int opd_floor_create(const opd_floor_config* cfg, int device_ordinal, opd_floor** out);
OPD_API void opd_floor_destroy(opd_floor* f);
OPD_API int opd_floor_info(const opd_floor* f, opd_floor_model_info* info);
/* `transform_batch` + `classify`: boxes_xywh [n][4] float32 (host for OPD_MEM_HOST, a device pointer read in place for OPD_MEM_DEVICE) ->
 * out [n] (host).  The foot point is (x + w / 2, y + h) in float64.  One upload, one launch, one download, one wait; n = 0 is OPD_OK. */
OPD_API int opd_floor_transform(opd_floor* f, const float* boxes_xywh, int n, int mem_kind, opd_floor_rec* out);
/* `transform_pixel` + `classify` of n camera points pts_xy [n][2] float64 (host): no foot-point step. */
OPD_API int opd_floor_transform_points(opd_floor* f, const double* pts_xy, int n, opd_floor_rec* out);
/* `classify_batch` of n floor points floor_xy [n][2] float64 (host) -> masks [n] (host). */
OPD_API int opd_floor_classify(opd_floor* f, const double* floor_xy, int n, uint64_t* masks);
/* opd_detr_detect_frames on host frames plus a floor record for every record of class `label`, computed while the records are on the
 * device from the box the Python shim derives, (x1, y1, float32(x2 - x1), float32(y2 - y1)).  `floor` = host [B][num_queries]; the row of
 * a record is its query_index; rows of queries without such a record are not written.  One host wait.  `m` and `f` must be on one device.
 * With opd_detr_set_nms on, the records are suppressed on the device first: rows are written for kept records only. */
OPD_API int opd_detr_detect_frames_floor(opd_detr* m, opd_floor* f, const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold,
                                         int label, opd_det* out, int32_t* counts, opd_floor_rec* floor);

/* ---- Tracker: the reference's `Tracker.update` per frame (fifth handle type: per-track state on the device, own stream) ----------------
 * DeepSORT-style tracking as src/tracking/tracker.py runs it once per frame: Kalman predict of every track, up to five association stages
 * (appearance, appearance + IoU behind a distance gate, IoU, the low-confidence rescue, tentative tracks), Kalman update with the
 * observation-centric re-update after an occlusion, new tracks, deletion after max_age frames.  The numeric state (Kalman x and P, last
 * observation, box, the last ten feature vectors) lives on the device for the life of the handle; slot list, ids and counters live in
 * the handle on the host.  One update is two launches and one host wait: the first launch predicts and writes three cost matrices, the host
 * solves the assignments over sub-blocks of them, the second launch commits and is not waited for (the next call orders behind it).
 * Arithmetic is float32 in a fixed order without fused multiply-adds; a track's numbers do not depend on how many other tracks or
 * detections there are, nor on its slot.  Which of several equally cheap assignments is taken is not specified. */
typedef struct opd_track opd_track; /* opaque tracker handle */

/* The reference's constructor keywords; a zeroed field means the reference's default.  What can therefore not be expressed: max_age = 0,
 * min_hits = 0 (the same as 1: a track is born with one hit), high_conf_threshold = 0 (use a tiny positive value), both weights zero
 * (the reference refuses that itself) and max_position_distance = 0 (its meaning there, "no gate", is spelled as a negative value). */
typedef struct opd_track_config {
    int32_t struct_size;          /* = sizeof(opd_track_config) */
    int32_t max_tracks;           /* slots: tracks alive at one time, 1 .. 1024 (0 = 128) */
    int32_t max_dets;             /* detections per update, 1 .. 1024 (0 = 128) */
    int32_t feature_dim;          /* width D of a feature vector, 1 .. 2048 (0 = 512) */
    int32_t max_age;              /* a track is dropped once it went this many frames without a match (0 = 30) */
    int32_t min_hits;             /* matches that confirm a track (0 = 3) */
    double iou_threshold;         /* (0 = 0.3) kept for the interface: the reference stores it and never reads it */
    double appearance_weight;     /* with motion_weight: both 0 = 0.7 and 0.3; otherwise they must sum to 1 within 1e-6 */
    double motion_weight;
    double max_position_distance; /* gate of the combined cost in pixels (0 = 150; negative = no gate) */
    double high_conf_threshold;   /* detections at or above start and match tracks, those below only rescue confirmed tracks (0 = 0.5) */
} opd_track_config;

typedef struct opd_track_rec {
    int32_t track_id, age, hits, time_since_update;
    float x[4];   /* Kalman state: position and velocity */
    float box[4]; /* xywh of the detection matched last */
} opd_track_rec;

typedef struct opd_track_status {
    int32_t max_tracks, max_dets, feature_dim, max_age, min_hits, device_ordinal;
    int32_t n_tracks, next_id;
    int32_t last_launches, last_waits; /* kernel launches and host waits of the last update */
} opd_track_status;

/* OPD_EINVAL, before the device is touched, for a size outside its range, a negative count or weights that do not sum to 1. */
OPD_API int opd_track_create(const opd_track_config* cfg, int device_ordinal, opd_track** out);
OPD_API void opd_track_destroy(opd_track* t);
/* Drop every track and start again at id 1, as `Tracker.reset`. */
OPD_API int opd_track_reset(opd_track* t);
OPD_API int opd_track_info(const opd_track* t, opd_track_status* info);
/* One frame.  boxes_xywh [n][4], foot_xy [n][2] (`camera_coords`), confidence [n]: host float32.  features [n][feature_dim] float32 or
 * NULL (no detection has one): host memory for OPD_MEM_HOST, device-accessible memory read by a device copy for OPD_MEM_DEVICE (it must be
 * complete before the call, and may be reused after it returns).  has_feature [n] (host) or NULL (every detection has one).  out_ids [n]
 * (host): the track id given to each detection, -1 where the reference leaves None (a low-confidence detection that rescued nothing).
 * n > max_dets is OPD_EINVAL and changes nothing.  More live tracks than max_tracks is OPD_EINVAL too: the frame then counts as one
 * without detections (every track aged, none matched or created), so the handle stays usable. */
OPD_API int opd_track_update(opd_track* t, const float* boxes_xywh, const float* foot_xy, const float* confidence, const float* features,
                             const uint8_t* has_feature, int feat_mem_kind, int n, int32_t* out_ids);
/* A run of F frames of one camera in ONE call with ONE host wait: what F calls of opd_track_update give, ids and state
 * bit for bit, with the association on the device between the frames (track_assoc_kernel: the host's five stages and the host's solver, pair for
 * pair, ties included).  The arrays are packed frame after frame: frame f occupies counts[f] rows, sum(counts) rows in all; out_ids likewise.
 * features NULL: no detection of any frame has one; has_feature NULL: every one has.  All detections are uploaded once; per frame the launches are
 * predict / cost, association, commit; then the ids and the track table come back and the handle adopts the table.  Afterwards opd_track_info
 * reports last_waits = 1 and last_launches = the launches that ran.  OPD_EINVAL before any device work, changing nothing: F <= 0, a negative count,
 * a counts[f] > max_dets, null counts, out_ids or frames_done.  A frame f that would exceed max_tracks counts as one without detections, as under
 * opd_track_update; the frames after it are NOT applied and their ids are -1, *frames_done = f + 1, and the call returns OPD_EINVAL: the state is
 * that of the per-frame loop that stopped at its error.  On success *frames_done = F. */
OPD_API int opd_track_update_sequence(opd_track* t, const float* boxes_xywh, const float* foot_xy, const float* confidence, const float* features,
                                      const uint8_t* has_feature, int feat_mem_kind, const int32_t* counts, int F, int32_t* out_ids,
                                      int32_t* frames_done);
/* opd_track_update_sequence for SEVERAL cameras in ONE call with ONE host wait: F frames in call order, frame f a frame of
 * trackers[camera_of[f]] (C distinct handles on one device, 1 <= C <= 64; they may differ in feature_dim, max_tracks, max_dets and every threshold).
 * The frames of one camera are taken in the order in which they appear; the cameras run side by side: step s of the call is the s-th frame of every
 * camera that has one, in at most four launches whatever C is (track_*_multi_kernel: the one-tracker kernels' code, a camera per blockIdx.y), so the
 * call takes as many steps as its longest camera has frames.  The arrays are packed frame after frame as above; a feature row is as wide as its
 * frame's own tracker's feature_dim.  Ids and states are those of one opd_track_update_sequence call per camera, bit for bit.  frames_done [C].
 * OPD_EINVAL before any device work, changing nothing: what opd_track_update_sequence refuses, a null list, C outside 1 .. 64, a camera_of entry
 * outside 0 .. C - 1, a null handle, a tracker named twice, a tracker that gets no frame, trackers on different devices.  A camera c that runs out
 * of slots at its frame f stops as under opd_track_update_sequence (that frame counts as one without detections, its later frames are not applied
 * and keep id -1, frames_done[c] = f + 1); every OTHER camera runs to its end and is adopted; the call returns OPD_EINVAL with that sentence for
 * the lowest-numbered stopped camera, naming it, and the list of all stopped cameras.  Afterwards opd_track_info reports on every tracker of the
 * call last_launches = the launches that ran for the call, and last_waits = 1 on trackers[0] (whose stream carried the call), 0 on the others. */
OPD_API int opd_track_update_streams(opd_track* const* trackers, int C, const int32_t* camera_of, int F, const float* boxes_xywh, const float* foot_xy,
                                     const float* confidence, const float* features, const uint8_t* has_feature, int feat_mem_kind,
                                     const int32_t* counts, int32_t* out_ids, int32_t* frames_done);
/* The live tracks in creation order: out [capacity], *count = how many there are (OPD_EINVAL when capacity is smaller; out may be NULL
 * with capacity 0 to ask for the count).  Waits for the last update's second launch. */
OPD_API int opd_track_get(opd_track* t, opd_track_rec* out, int capacity, int* count);

/* Detection and tracking in ONE call with ONE host wait: the frame-list detect call with the suppression of
 * opd_detr_set_nms, the feature stage of `feature_kind`, and one tracker update per frame, frame b into trackers[b] (B distinct handles:
 * one camera each).  The kept records and their feature rows enter the tracker where they lie on the device; no feature row is returned.
 * Records and counts come back as from opd_detr_detect_frames with the suppression on.  track_ids [B][num_queries]: the id of kept record
 * i of frame b at [b * num_queries + i], -1 where opd_track_update writes -1; entries at i >= counts[b] are not written.  n_featured [B]:
 * how many of the frame's kept records entered with a feature row: counts[b] for ENCODER and COLOR, 0 for NONE, for REID the number that
 * got one of the `slots` crop slots (handed out in frame, score order; a record beyond them enters with has_feature = 0).  `r` and `slots`
 * are read for REID only.  OPD_EINVAL before any device work: a null handle or output; the suppression off on `m`, or on for another label;
 * one tracker named twice; a handle on another device; a tracker with max_dets < num_queries, or with a feature_dim other than the kind's
 * row width (256 for ENCODER and COLOR, the Re-ID model's for REID); REID with r == NULL or slots outside 1 .. max_crops; ENCODER or COLOR
 * with d_model != 256; COLOR with a frame edge above 4096; an unknown kind; and what opd_detr_detect_frames refuses.  A tracker that would
 * exceed max_tracks behaves as under opd_track_update: records and counts are delivered, its ids are all -1, the frame counts as one
 * without detections, the call returns OPD_EINVAL, and the other trackers of the batch are committed.  Afterwards opd_track_info reports
 * last_waits = 0 (the wait was the detector's) and last_launches = the ingest, predict and commit launches that ran. */
#define OPD_TRACK_FEAT_NONE 0    /* motion only: the tracker sees features == NULL */
#define OPD_TRACK_FEAT_ENCODER 1 /* the ROI rows of opd_detr_detect_frames_features (D = 256) */
#define OPD_TRACK_FEAT_COLOR 2   /* the colour-histogram rows of opd_detr_detect_frames_color (D = 256) */
#define OPD_TRACK_FEAT_REID 3    /* the rows of `r` (D = its feature_dim), planned as opd_detr_detect_frames_reid plans them */
OPD_API int opd_detr_detect_frames_track(opd_detr* m, opd_reid* r, opd_track* const* trackers, const uint8_t* const* frames, int B, int h,
                                         int w, int H, int W, float threshold, int label, int feature_kind, int slots, opd_det* out,
                                         int32_t* counts, int32_t* track_ids, int32_t* n_featured);
/* opd_detr_detect_frames_track for B CONSECUTIVE frames of ONE camera into ONE tracker, in frame order: one batched forward,
 * suppression and feature stage; then per frame, on the detector's stream, ingest, predict / cost, association on the device and commit; ONE host
 * wait; no matrix, box or feature row crosses the bus.  Records, counts, track_ids [B][num_queries] and n_featured [B] as above; for REID the
 * `slots` crop slots are per call, handed out in (frame, score) order.  The refusals are those of opd_detr_detect_frames_track, in the same order.
 * Out of slots at frame f: as opd_track_update_sequence (records and counts of all B frames are still delivered).  *frames_done = B on success.
 * Afterwards opd_track_info reports last_waits = 0 and last_launches = the launches that ran. */
OPD_API int opd_detr_detect_sequence_track(opd_detr* m, opd_reid* r, opd_track* t, const uint8_t* const* frames, int B, int h, int w, int H, int W,
                                           float threshold, int label, int feature_kind, int slots, opd_det* out, int32_t* counts,
                                           int32_t* track_ids, int32_t* n_featured, int32_t* frames_done);
/* opd_detr_detect_sequence_track for SEVERAL cameras: B frames in call order, frame b a frame of trackers[camera_of[b]]
 * (C distinct handles, 1 <= C <= 64, every one with a frame).  One batched forward, suppression and feature stage over all B frames; then, on the
 * detector's stream in front of the ONE host wait, the steps of opd_track_update_streams with an ingest launch in front of each.  Records, counts,
 * track_ids [B][num_queries] and n_featured [B] are what one opd_detr_detect_sequence_track call per camera gives (the `frame` member of a record
 * is its position in THIS call); for REID the `slots` crop slots are per call, in (frame, score) order.  The refusals are those of
 * opd_detr_detect_frames_track per tracker, in the same order, then those of opd_track_update_streams for the list.  Out of slots in camera c: as
 * opd_track_update_streams, frames_done [C] (records and counts of all B frames are still delivered).  Afterwards opd_track_info reports
 * last_waits = 0 and last_launches = the launches that ran for the call, on every tracker. */
OPD_API int opd_detr_detect_streams_track(opd_detr* m, opd_reid* r, opd_track* const* trackers, int C, const int32_t* camera_of,
                                          const uint8_t* const* frames, int B, int h, int w, int H, int W, float threshold, int label, int feature_kind,
                                          int slots, opd_det* out, int32_t* counts, int32_t* track_ids, int32_t* n_featured, int32_t* frames_done);
/* opd_detr_detect_tiled with the colour-feature, floor and track stages on the MERGED records, all on the detector's stream in front of the call's
 * ONE host wait (DESIGN.md sections 7a, 7k): what detect_tiled + opd_color_features + opd_floor_transform + opd_track_update give in four calls.
 * With S = n_tiles x num_queries, the feature, floor and track-id row of merged record k of frame f is row f x S + k -- by POSITION, since two
 * tiles of a frame use the same query numbers; rows at or behind counts[f] are unspecified.  Arithmetic, operation for operation that of the
 * separate calls: a box is x, y, w, h each rounded from float64 to float32 ONCE; the colour crop is cut from the whole frame f with those four
 * floats (widened back; the width is not re-derived); the floor foot point is taken from the rounded box; the tracker's foot point is
 * (x + w / 2, y + h) in float64 from the UNROUNDED doubles, then rounded to float32; the confidence is the record's score.
 *   feature_kind  OPD_TRACK_FEAT_NONE or OPD_TRACK_FEAT_COLOR (256 numbers per row)
 *   features      NULL, or host [n_frames][S][256]: the rows to the caller (with trackers and NULL here no row leaves the device)
 *   floor         NULL, or a floor-map handle; floor_out host [n_frames][S]
 *   trackers      NULL, or [n_frames] distinct handles, frame f into trackers[f]; track_ids host [n_frames][S] (-1 where opd_track_update writes
 *                 -1), n_featured host [n_frames]: counts[f] with COLOR, 0 with NONE.  A tracker out of slots: as opd_detr_detect_frames_track.
 * OPD_EINVAL before any device call, besides everything opd_detr_detect_tiled refuses: NULL `stages` or a wrong struct_size; another
 * feature_kind (a box merged from two tiles' maps has no encoder row; Re-ID is the entry opd_detr_detect_tiled_reid below); `features` with FEAT_NONE; COLOR on a frame
 * with a side above 4096 or a handle with d_model != 256; floor_out NULL with `floor`, a floor map on another device; track_ids or n_featured
 * NULL with `trackers`; a NULL tracker, one on another device, one named twice, one with max_dets < S, one with feature_dim != 256 under COLOR. */
typedef struct opd_tile_stages {
    int32_t struct_size;  /* = sizeof of this struct */
    int32_t feature_kind;
    float* features;
    opd_floor* floor;
    opd_floor_rec* floor_out;
    opd_track* const* trackers;
    int32_t* track_ids;
    int32_t* n_featured;
} opd_tile_stages;
OPD_API int opd_detr_detect_tiled_stages(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw,
                                         int n_tiles, int H, int W, float threshold, const opd_tile_params* p, const opd_tile_stages* stages,
                                         opd_tile_det* out, int32_t* counts);
/* opd_detr_detect_tiled with the Re-ID rows of the MERGED records inside the call (DESIGN.md sections 7a, 7k): what detect_tiled +
 * opd_reid_extract (+ opd_floor_transform + opd_track_update) give in separate calls, behind the call's ONE host wait.  The crops are planned on the
 * device from the merged records and cut from the WHOLE frames where the source step left them (the tile windows play no part); the Re-ID forward runs
 * on the Re-ID handle's own stream between two events, and the call holds that handle for its duration.  With S = n_tiles x num_queries:
 *   slots      crop slots of the call, 1 .. max_crops of `reid`.  They go to the merged records in (frame, position) order, within a frame the
 *              merge's own descending-score order.  *n_person = the merged records of the call (the sum of the counts; it may exceed slots, which
 *              is no error); rows and slot_map entries at k >= min(*n_person, slots) are not written
 *   slot_map   host [slots]: row k belongs to merged record slot_map[k] = f x S + position
 *   features   host [slots][feature_dim], or NULL with trackers (then no row leaves the device).  A record's box is x, y, w, h each rounded from
 *              float64 to float32 ONCE and widened back (the width is not re-derived); row k equals, bit for bit, the row opd_reid_extract
 *              returns on the same handle for that frame and that float32 box
 *   floor, floor_out, trackers, track_ids, n_featured   as in opd_tile_stages, rows by position: the floor foot point from the rounded box, the
 *              tracker's from the unrounded doubles.  The Re-ID rows enter the trackers where the forward left them; a record beyond the slots
 *              enters with has_feature = 0; n_featured[f] = the records of frame f that got a slot.  A tracker out of slots: as
 *              opd_detr_detect_frames_track.
 * OPD_EINVAL before any device call, besides everything opd_detr_detect_tiled refuses: NULL `stages` or a wrong struct_size; NULL `reid`, slots
 * outside 1 .. max_crops, a Re-ID handle on another device; NULL slot_map or n_person; NULL `features` without trackers; floor_out NULL with
 * `floor`, a floor map on another device; track_ids or n_featured NULL with `trackers`; a NULL tracker, one on another device, one named twice,
 * one with max_dets < S, one whose feature_dim differs from the Re-ID model's. */
typedef struct opd_tile_reid_stages {
    int32_t struct_size;  /* = sizeof of this struct */
    int32_t slots;
    opd_reid* reid;
    float* features;
    int32_t* slot_map;
    int32_t* n_person;
    opd_floor* floor;
    opd_floor_rec* floor_out;
    opd_track* const* trackers;
    int32_t* track_ids;
    int32_t* n_featured;
} opd_tile_reid_stages;
OPD_API int opd_detr_detect_tiled_reid(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw,
                                       int n_tiles, int H, int W, float threshold, const opd_tile_params* p, const opd_tile_reid_stages* stages,
                                       opd_tile_det* out, int32_t* counts);
/* opd_detr_detect_tiled for a grid whose tiles DIFFER in size (a grid with interior tiles at the default overlap, a frame side that does not
 * divide): `tile_HW` [n_tiles][2] is the model size of each tile, where the other entries take one H x W.  Each frame is uploaded once; tile t is
 * resampled from its window to tile_HW[t] into the top-left corner of a canvas of max H x max W with zeros around it (byte for byte the canvas of
 * opd_detr_detect_ragged's caller: Pillow's resize of contiguous copies of the windows), the forward runs as a ragged batch with
 * valid_hw = tile_HW (eagerly, as every ragged batch), the boxes of tile t are scaled to ITS window, and the suppression, merge and wait are
 * those of opd_detr_detect_tiled.  Windows of one size with one model size take that entry's path, with its records byte for byte.
 * `stages`: NULL, or the colour-feature, floor and track stages on the merged records exactly as in opd_detr_detect_tiled_stages (rows by
 * position).  Re-ID rows are refused here (feature_kind OPD_TRACK_FEAT_REID): for such a grid they are the entry opd_detr_detect_tiled_ragged_reid below.
 * OPD_EINVAL before any device call: everything opd_detr_detect_tiled (with `stages`: opd_detr_detect_tiled_stages) refuses except windows of
 * more than one size; NULL `tile_HW`; a model size below 1; a canvas outside the handle's maximum. */
OPD_API int opd_detr_detect_tiled_ragged(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw,
                                         int n_tiles, const int32_t* tile_HW, float threshold, const opd_tile_params* p,
                                         const opd_tile_stages* stages, opd_tile_det* out, int32_t* counts);
/* opd_detr_detect_tiled_reid for a grid whose tiles DIFFER in size: the source step, forward and records of opd_detr_detect_tiled_ragged (`tile_HW`
 * [n_tiles][2] as there), and behind the seam merge the Re-ID, floor and track stages exactly as documented for opd_detr_detect_tiled_reid: slots,
 * slot_map, rows by slot, floor and track-id rows by position, crops cut from the WHOLE frames (the windows and their sizes play no part).  Windows of
 * one size with one model size take opd_detr_detect_tiled_reid's path and give its bytes.
 * OPD_EINVAL before any device call: everything opd_detr_detect_tiled_ragged (without stages) and opd_detr_detect_tiled_reid refuse, except windows
 * of more than one size. */
OPD_API int opd_detr_detect_tiled_ragged_reid(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw,
                                              int n_tiles, const int32_t* tile_HW, float threshold, const opd_tile_params* p,
                                              const opd_tile_reid_stages* stages, opd_tile_det* out, int32_t* counts);
/* The solver of the association on its own (host only): cost [rows][cols] row-major -> row_to_col [rows], -1 for a row left alone;
 * min(rows, cols) pairs of smallest total cost, as scipy.optimize.linear_sum_assignment. */
OPD_API int opd_assign(const double* cost, int rows, int cols, int32_t* row_to_col);

/* ---- Hybrid tracker: the reference's `LightweightTracker` (sixth handle type: per-track state and flow points on the device) ------------
 * src/tracking/lightweight_tracker.py:211-455 as the reference's shipped configuration runs it (`tracking.hybrid_mode`): a detection frame
 * goes through `update_with_detections` (Kalman predict, greedy IoU matching, Kalman update, new tracks, deletion after max_age frames,
 * the flow points of `OpticalFlowTracker.initialize`), every frame in between through `interpolate` (pyramidal Lucas-Kanade on the box
 * centres, Kalman update of the tracks whose point was followed, Kalman predict of the others).  Each is ONE call with one host wait, and
 * no track number is computed on the host: tracks, ids, counters, the next id and the point list live on the device; the calls return
 * ids and boxes.  The handle owns a flow handle and runs its gray, pyramid and LK launches on the same stream as its own two kernels.
 * Arithmetic: P, S and K in float32, x in float32 until the first detection-frame match and in float64 from then on (what numpy's
 * promotion makes of the reference's `KalmanFilter.update` with a float64 centre), IoU in float64, in a fixed order without fused
 * multiply-adds; a track's numbers do not depend on the other tracks or on its position. */
typedef struct opd_lwt opd_lwt; /* opaque hybrid-tracker handle */

typedef struct opd_lwt_config {
    int32_t struct_size;      /* = sizeof of this struct */
    int32_t max_tracks;       /* tracks alive at one time, 1 .. 1024 (0 = 256) */
    int32_t max_dets;         /* detections per update, and flow points, 1 .. 1024 (0 = 256) */
    int32_t max_age;          /* a track is dropped once time_since_update exceeds this (0 = 30) */
    int32_t use_optical_flow; /* 0: `interpolate` predicts every track and no frame is read */
    int32_t reserved[3];      /* zero */
    double iou_threshold;     /* matching stops below this IoU (0 = 0.3).  Negative is refused: the reference's loop would never end */
    opd_flow_config flow;     /* frame limits and LK parameters as for the flow handle; max_points is ignored (max_dets is used) */
} opd_lwt_config;

typedef struct opd_lwt_rec {
    int32_t track_id, reserved;
    double bbox[4]; /* xywh */
} opd_lwt_rec;

typedef struct opd_lwt_track {
    int32_t track_id, age, hits, time_since_update;
    int32_t x_is_float32; /* 1: x holds float32 values and is still computed on in float32 */
    int32_t reserved;
    double bbox[4];       /* xywh (float32 values) */
    double center[2];
    double x[4];          /* Kalman state: position and velocity */
    float P[16];          /* covariance, row-major */
} opd_lwt_track;

typedef struct opd_lwt_status {
    int32_t max_tracks, max_dets, max_age, use_optical_flow, device_ordinal;
    int32_t n_tracks, next_id, n_points; /* n_points: flow points held (`prev_points`) */
    int32_t last_launches, last_waits;   /* kernel launches and host waits of the last update or interpolate call */
    double iou_threshold;
} opd_lwt_status;

/* OPD_EINVAL, before the device is touched, for a size outside its range, a negative max_age or iou_threshold, a wrong struct_size. */
OPD_API int opd_lwt_create(const opd_lwt_config* cfg, int device_ordinal, opd_lwt** out);
OPD_API void opd_lwt_destroy(opd_lwt* t);
/* Drop every track and point and start again at id 1, as `LightweightTracker.reset`. */
OPD_API int opd_lwt_reset(opd_lwt* t);
OPD_API int opd_lwt_info(const opd_lwt* t, opd_lwt_status* info);
/* `update_with_detections`.  boxes_xywh [n][4] host float32; ids_out [n] host: the track id of every detection.  `bgr` [h][w][3] uint8 is
 * the frame the points will be followed FROM: host memory or a device pointer read in place, as for the flow handle; without optical
 * flow it is not read and may be NULL.  n > max_dets is OPD_EINVAL before anything is launched.  New tracks that would not fit beside
 * the live ones are OPD_EINVAL too: the kernel finds that out after matching and before it writes, so tracks, ids, points and the
 * reference frame are left as they were. */
OPD_API int opd_lwt_update(opd_lwt* t, const uint8_t* bgr, int mem_kind, int h, int w, const float* boxes_xywh, int n, int32_t* ids_out);
/* `interpolate`: recs_out [capacity] host, *count records, one per live track in creation order (OPD_EINVAL when capacity is smaller;
 * *count then says how many there are). */
OPD_API int opd_lwt_interpolate(opd_lwt* t, const uint8_t* bgr, int mem_kind, int h, int w, opd_lwt_rec* recs_out, int capacity, int* count);
/* F calls of opd_lwt_interpolate on frames[0 .. F) behind ONE host wait: records, states, ids and the counts of opd_lwt_info afterwards
 * are those of the per-frame loop, bit for bit.  recs_out [F][capacity] host and counts [F]: frame f's records at recs_out + f * capacity,
 * counts[f] of them (the number of live tracks, the same for every frame).  Per frame, on the handle's stream: gray, pyramid, LK and the
 * track kernel; the two pyramids alternate, the LK launches are sized for the points held at entry while the device-resident count decides
 * which of their waves work, and all records travel in one download.  All frames have the size h x w and the same mem_kind; host frames are
 * uploaded from where they lie and must stay unchanged until the call returns.  Without optical flow no frame is read and `frames` may be
 * NULL.  As in the per-frame call, a handle that holds no points at entry reads no frame either.  OPD_EINVAL before any device work: F
 * outside 1 .. 64; capacity below the handle's max_tracks; whatever opd_lwt_interpolate refuses for one of the frames. */
OPD_API int opd_lwt_interpolate_sequence(opd_lwt* t, const uint8_t* const* frames, int mem_kind, int F, int h, int w, opd_lwt_rec* recs_out,
                                         int capacity, int32_t* counts);
/* A detection frame of the hybrid tracker INSIDE the detect call: opd_detr_detect_frames (suppression on) followed, per frame b, by
 * opd_lwt_update(trackers[b], frames[b], the kept records' boxes), with ONE host wait for all of it and bit for bit the same ids, track
 * states, flow points and reference frame.  B distinct handles, one camera each.  Behind the suppression, per tracker, on the detector's
 * stream: an ingest launch writes the kept records as the float32 xywh boxes the per-frame path hands over (corners as they are, width
 * and height as differences in double, rounded once) and leaves their count on the device; gray and pyramid are built from the
 * camera-resolution frame where the detector's source step put it (no second upload); the update kernel reads the count on the device.
 * The ids and every tracker's head travel in the call's one fetch.  out / counts: as from opd_detr_detect_frames.  track_ids
 * [B][num_queries]: the id of kept record i of frame b at [b][i]; entries at i >= counts[b] are not written.  No feature rows.
 * OPD_EINVAL before any device work: a null handle or output; opd_detr_set_nms off on `m`, or on for another label; a tracker named
 * twice, on another device, or made with max_dets < num_queries; with optical flow, a frame larger than a tracker was made for; whatever
 * opd_detr_detect_frames refuses.  New tracks that do not fit (as under opd_lwt_update): that tracker's state, points and reference
 * frame are as before and its ids are all -1; records and counts are delivered, the other trackers are committed, and the call returns
 * OPD_EINVAL.  The trackers' last_waits is 0 afterwards: the wait is the detector's. */
OPD_API int opd_detr_detect_frames_hybrid(opd_detr* m, opd_lwt* const* trackers, const uint8_t* const* frames, int B, int h, int w, int H,
                                          int W, float threshold, int label, opd_det* out, int32_t* counts, int32_t* track_ids);
/* A run of F consecutive frames of ONE camera, key frames (is_key[f] != 0: detection frames) and in-between frames, with ONE host wait:
 * what the per-frame loop of opd_detr_detect_frames + opd_lwt_update on the key frames and opd_lwt_interpolate on the others gives, bit for
 * bit.  The K key frames (K <= max_batch; K = 0 is opd_lwt_interpolate_sequence and runs no forward) go through ONE batched forward,
 * suppression included.  Then, in frame order on the detector's stream: a key frame runs ingest, gray + pyramid and the update; an
 * in-between frame is uploaded from where it lies (host memory) and runs gray + pyramid, LK and the track kernel.  The LK launches are
 * sized for the points held at entry in front of the first key frame and for num_queries behind it; the device-resident count decides.
 * The first frame need not be a key frame.  out [K][num_queries], counts [K], track_ids [K][num_queries]: per key frame, as from
 * opd_detr_detect_frames_hybrid.  recs_out [F - K][capacity], rec_counts [F - K]: per in-between frame, as from
 * opd_lwt_interpolate_sequence.  *frames_done = F on success, and a per-frame or another sequence call afterwards continues bit for bit.
 * A key frame f whose new tracks do not fit changes nothing, as under opd_lwt_update, and ends the run: the update kernel raises a sticky
 * word on the device at which every launch of the frames behind it leaves at once, so the tracker (state, points, reference frame) is
 * that of the per-frame loop that stopped at its error.  *frames_done = f + 1, the ids of frame f and of later key frames are -1, the
 * record counts of later in-between frames are 0, the records and counts of ALL key frames are delivered, and the call returns
 * OPD_EINVAL.  OPD_EINVAL before any device work: whatever opd_lwt_interpolate_sequence and opd_detr_detect_frames_hybrid refuse. */
OPD_API int opd_detr_detect_sequence_hybrid(opd_detr* m, opd_lwt* t, const uint8_t* const* frames, const uint8_t* is_key, int F, int h, int w,
                                            int H, int W, float threshold, int label, opd_det* out, int32_t* counts, int32_t* track_ids,
                                            opd_lwt_rec* recs_out, int capacity, int32_t* rec_counts, int32_t* frames_done);
/* A detection frame of the hybrid tracker INSIDE a tiled call (DESIGN.md sections 7a, 7k, 7n).  With S = n_tiles x num_queries, per frame f the
 * result equals, bit for bit, three steps: opd_detr_detect_tiled (`tile_HW` given: opd_detr_detect_tiled_ragged); opd_lwt_update(trackers[f],
 * frames[f], boxes) with the boxes of the MERGED records, x, y, w, h each rounded from float64 to float32 ONCE (np.array([d.bbox ...], float32));
 * and, with `floor`, opd_floor_transform as in opd_detr_detect_tiled_stages -- ids, every number of every track, the counts of opd_lwt_info, flow
 * points and reference frame, merged records and counts, behind ONE host wait.  Behind the seam merge, per tracker, on the detector's stream: the
 * ingest launch reads the merged records where the merge left them and clamps their device-resident count to S; gray and pyramid are built from the
 * WHOLE h x w frame where the tiled source uploaded it (no second upload; no tile plays a part); the update kernel reads the count on the device.
 *   tile_HW    NULL: tiles of one size at one model size H x W.  Else [n_tiles][2], the model size of each tile; H and W are ignored
 *   trackers   [n_frames] distinct handles, frame f into trackers[f]
 *   track_ids  host [n_frames][S], by POSITION: the id of merged record k of frame f at [f][k]; entries at k >= counts[f] are not written
 *   floor      NULL, or a floor-map handle; floor_out host [n_frames][S], rows by position
 * OPD_EINVAL before any device work: everything the plain tiled entry (uniform or ragged) refuses; NULL `hy` or a wrong struct_size; NULL trackers
 * or track_ids; a tracker that is NULL, named twice, on another device, made with max_dets < S, or (with optical flow) made for frames smaller than
 * h x w; floor_out NULL with `floor`, a floor map on another device.  New tracks that do not fit: as in opd_detr_detect_frames_hybrid (that tracker
 * is left as it was and its ids are -1; records and counts are delivered, the other trackers are committed, the call returns OPD_EINVAL).  The
 * trackers' last_waits is 0 afterwards: the wait is the detector's. */
typedef struct opd_tile_hybrid {
    int32_t struct_size, reserved; /* sizeof of this struct; zero */
    opd_lwt* const* trackers;
    int32_t* track_ids;
    opd_floor* floor;
    opd_floor_rec* floor_out;
} opd_tile_hybrid;
OPD_API int opd_detr_detect_tiled_hybrid(opd_detr* m, const uint8_t* const* frames, int n_frames, int h, int w, const int32_t* tiles_yxhw,
                                         int n_tiles, int H, int W, const int32_t* tile_HW, float threshold, const opd_tile_params* p,
                                         const opd_tile_hybrid* hy, opd_tile_det* out, int32_t* counts);
/* opd_detr_detect_sequence_hybrid with TILED key frames: a run of F consecutive h x w frames of one camera.  The K key frames go through ONE tiled
 * forward (K x n_tiles <= max_batch; `tile_HW` as above), suppression and seam merge.  Then, in frame order on the detector's stream: a key frame
 * runs ingest (merged records of key frame k), gray + pyramid of its whole frame and the update; an in-between frame is uploaded from where it lies
 * and runs gray + pyramid, LK and the track kernel.  The LK launches behind the first key frame are sized for S = n_tiles x num_queries points.  out
 * [K][S], counts [K], track_ids [K][S]: per key frame, as from opd_detr_detect_tiled_hybrid; recs_out, capacity, rec_counts, frames_done, the
 * sticky word at a key frame whose new tracks do not fit, and K = 0 (opd_lwt_interpolate_sequence; no forward, the windows are not read): as in
 * opd_detr_detect_sequence_hybrid.  Results equal the per-frame loop of opd_detr_detect_tiled_hybrid's three steps and opd_lwt_interpolate, bit for
 * bit.  OPD_EINVAL before any device work: whatever opd_detr_detect_sequence_hybrid and the plain tiled entry refuse; max_dets < S. */
OPD_API int opd_detr_detect_tiled_sequence_hybrid(opd_detr* m, opd_lwt* t, const uint8_t* const* frames, const uint8_t* is_key, int F, int h, int w,
                                                  const int32_t* tiles_yxhw, int n_tiles, int H, int W, const int32_t* tile_HW, float threshold,
                                                  const opd_tile_params* p, opd_tile_det* out, int32_t* counts, int32_t* track_ids,
                                                  opd_lwt_rec* recs_out, int capacity, int32_t* rec_counts, int32_t* frames_done);
/* The live tracks in creation order (out may be NULL with capacity 0 to ask for the count).  A read-back for inspection: one more wait. */
OPD_API int opd_lwt_get(opd_lwt* t, opd_lwt_track* out, int capacity, int* count);

/* Thread-local description of the last error returned on this thread ("" if none). */
OPD_API const char* opd_last_error(void);

/* Library / kernel build identification, e.g. "opd_hip 0.1 gfx950". */
OPD_API const char* opd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OPD_DETR_H */
