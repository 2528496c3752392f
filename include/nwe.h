/*
 * nwe.h -- C ABI of the MI355X-native NeRF volume-rendering path (libnwe_hip.so).
 *
 * The reference (dmjovan/NeRF-Workspaces-Explorer) has no FFI layer: its hot path is plain PyTorch
 * behind the public surface of NeRFReplicaInferenceHandler.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  Plain pointers and sizes
 * only; no torch types.  All functions return 0 on success, a NWE_ERR_* code otherwise, never throw,
 * and leave a message retrievable with nwe_last_error().  A context is not thread-safe.
 */
#ifndef NWE_H
#define NWE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nwe_ctx nwe_ctx;

enum {
    NWE_OK = 0,
    NWE_ERR_INVALID = 1,     /* bad argument (null pointer, size, shape) */
    NWE_ERR_UNSUPPORTED = 2, /* network shape / precision combination has no kernel */
    NWE_ERR_HIP = 3,         /* a HIP runtime call failed; message holds hipGetErrorString */
    NWE_ERR_STATE = 4        /* call order: network / sampling tables not set */
};

enum { NWE_NET_COARSE = 0, NWE_NET_FINE = 1 };

/* Arithmetic of the MLP GEMMs.  Everything else (rays, sampling, encoding, compositing) is fp32
 * (with the fp64 running products/sums torch's CPU cumprod/cumsum use) in every mode. */
enum {
    NWE_PREC_F16X3 = 0, /* MFMA f16, operands split hi+lo, 3 products, fp32 accumulate: fp32-grade (default) */
    NWE_PREC_F16X1 = 1, /* MFMA f16 single product: ~1e-3 abs on RGB, PSNR > 50 dB */
    NWE_PREC_F32 = 2    /* fp32 FMA chain on the vector ALU, any layer shape: on-device reference */
};

/* bits OR-ed into *nwe_outputs.flags: the reference only prints
 * "[Numerical Error] <key> contains NaN or inf." (nerf_replica_inference_handler.py:273-275)
 * NWE_FLAG_RGB_COARSE is not raised by a render of pinhole views on the folded MFMA path (the default for networks with view
 * directions) that requests nothing but rgb / depth / acc / flags, sets no test hook and has n_importance > 0: such a call
 * evaluates only the density of the coarse samples (their weights are all the fine pass reads), so there is no coarse colour
 * to check.  Exception: networks whose skip input enters the last trunk layer (6 deep with skips (4,)) still compute the
 * coarse colour and report it.  Every other bit means what it means in any call.
 * fp16 range (NWE_PREC_F16X3 / F16X1): hidden activations are split into fp16 hi + lo, so an activation of 65520 or more (hi =
 * inf) cannot be represented.  The MFMA kernels keep the resulting NaN through their ReLUs and the compositing's relu(sigma), so
 * such a call raises NWE_FLAG_RAW (when raw outputs are requested) and the rgb / depth / acc bits instead of returning finite,
 * wrong values.  NWE_PREC_F32 has no such limit.
 * Non-finite and degenerate inputs are defined as in the reference, whose PyTorch code runs on anything: every output's NaN /
 * inf pattern is the reference's and the bits below report it (tests/input_domain.py lists the cases).  In particular
 *   - a NaN weight or bias stays NaN through every ReLU of every precision, NWE_PREC_F32 included (torch's relu keeps it);
 *   - z_std of a ray with NaN or inf importance samples is NaN, as torch.std's, and raises NWE_FLAG_ZSTD; sample_cond /
 *     sample_amp / sample_switch keep a NaN the way torch's min / max do; with finite coarse depths NaN samples are the last
 *     entries of z_fine, behind every depth, as torch.sort leaves them (with NaN or inf coarse depths - far = inf, NaN bounds -
 *     every entry is non-finite as in the reference, in an order that is not specified);
 *   - coordinate range of the positional encoding (NWE_PREC_F16X3 / F16X1): gamma(x) is guaranteed for |x / 10| * 32 < 1.6e6,
 *     i.e. point coordinates below 5e5 (nwe_selftest report[7]).  Beyond that, and for inf or NaN, the encoding is NaN - never
 *     a finite wrong value - and so are the raw outputs and rgb / depth / acc of the ray, with their bits; the identity inputs
 *     x / 10 are split into fp16 hi + lo and end at 65520 in the same way.  NWE_PREC_F32 (sinf / cosf) is defined for every
 *     finite coordinate.
 * near <= far: nwe_render, nwe_create_rays and nwe_render_tiled refuse far < near with NWE_ERR_INVALID (near == far, inf and
 * NaN bounds are rendered as the reference renders them).  For nwe_render_rays near <= far on every ray is a PRECONDITION: the
 * fine pass merges the coarse depths with the importance samples as two ascending lists where the reference sorts their
 * union, so with far < near its sample order - and every fine output - differs from the reference's.
 * Camera domain of nwe_render, nwe_create_rays and nwe_render_tiled: fx, fy, cx and cy are four independent floats.  Any
 * finite non-zero fx and fy (negative focal lengths mirror the image along their axis), any finite cx and cy (on a pixel,
 * between pixels, outside the image) and any finite upper 3x4 part of c2w (a rotation or any other linear map, any
 * translation) give rays that are the reference's bit for bit, zero signs included: x = (w - cx) / fx and y = (h - cy) / fy
 * are true fp32 divisions, d = R (x, y, 1) is summed left to right without FMA onto torch's +0 accumulator (three products
 * that are all -0 give +0, not -0).  Row 3 of c2w is ignored, whatever it holds.
 * fx == 0 or fy == 0 (either sign of zero) is refused by all three with NWE_ERR_INVALID before anything is queued: the
 * outputs stay untouched and nwe_last_kernel_ms / nwe_last_launch_parts keep describing the previous launch.
 * (tests/camera_domain.py lists the cases.) */
enum {
    NWE_FLAG_RGB = 1u << 0, NWE_FLAG_DEPTH = 1u << 1, NWE_FLAG_ACC = 1u << 2, NWE_FLAG_DISP = 1u << 3,
    NWE_FLAG_RGB_COARSE = 1u << 4, NWE_FLAG_DEPTH_COARSE = 1u << 5, NWE_FLAG_ACC_COARSE = 1u << 6,
    NWE_FLAG_DISP_COARSE = 1u << 7, NWE_FLAG_RAW = 1u << 8, NWE_FLAG_ZSTD = 1u << 9
};

/* Device output buffers, owned by the caller; any pointer may be NULL (that output is skipped).
 * R = number of rays of the call, S = n_samples + n_importance.  Keys mirror the output dict of
 * NeRFReplicaInferenceHandler._volumetric_rendering (nerf_replica_inference_handler.py:256-268).
 * When n_importance == 0 the "fine" slots receive the coarse results (the reference raises
 * UnboundLocalError there, :263). */
typedef struct nwe_outputs {
    uint64_t struct_bytes; /* = sizeof(nwe_outputs): a caller built against another version of this header (fields were
                              added since) is refused with NWE_ERR_INVALID instead of having pointers misread */
    float *rgb;          /* [R,3]   rgb_fine    */
    float *depth;        /* [R]     depth_fine  */
    float *acc;          /* [R]     acc_fine    */
    float *disp;         /* [R]     disp_fine   */
    float *z_std;        /* [R]     z_std       */
    float *rgb_coarse;   /* [R,3]               */
    float *depth_coarse; /* [R]                 */
    float *acc_coarse;   /* [R]                 */
    float *disp_coarse;  /* [R]                 */
    float *raw_coarse;   /* [R,n_samples,4]  network output, [rgb_raw(3), sigma_raw] */
    float *raw_fine;     /* [R,S,4]             */
    float *z_fine;       /* [R,S]  sorted sample depths of the fine pass (handler.py:243) */
    float *weights_coarse; /* [R,n_samples]  alpha * transmittance of the coarse pass: the 4th return value of raw2outputs
                                   (nerf/models/model_utils.py:80), whose [..., 1:-1] slice is what sample_pdf takes
                                   (handler.py:237) */
    /* Conditioning diagnostics of the importance sampling (nerf/rays/rays.py:103-119), one value per ray, taken over
     * the importance samples that are interpolated between two different cdf entries (the clamped end case
     * below == above, :104-105, has a structural denom of 0 and a zero-width bin and is left out): */
    float *sample_cond;  /* [R]    smallest cdf step `denom` (:113) BEFORE the `denom < 1e-5 -> 1` replacement (:114); a value
                                   below 1e-5 says that a sample of this ray went through the replacement (1.0 if none) */
    float *sample_amp;   /* [R]    largest bin_width / denom (denom after the replacement): a sample depth moves by this
                                   much per unit change of the coarse cdf, i.e. the first-order amplification of a
                                   rounding difference in the coarse weights IN THE REFERENCE ALGORITHM ITSELF */
    float *sample_switch;/* [R]    smallest |denom - 1e-5| before the replacement: the distance of the ray's samples
                                   from the discontinuity of :114 */
    float *feat_map;     /* [R,W/2] feat_map_fine (experiment.endpoint_feat, handler.py:248-254,270-271): the view layer's outputs
                                   of the FINE pass composited like rgb (model_utils.py:87-89; the reference takes the last 128
                                   channels, i.e. W = 256).  NWE_PREC_F32 only, networks with view directions, n_importance > 0 */
    uint32_t *flags;     /* [1]    NWE_FLAG_* bits, OR-ed (caller zeroes it) */
} nwe_outputs;

/* Create a context bound to HIP device `device`.  device == -1 creates a host-only context that can
 * pack networks (for CPU tests of the packer) but cannot render.
 * Replaces: NeRFReplicaInferenceHandler.__init__ device side (handler.py:25-86). */
int nwe_create(nwe_ctx **out, int device);
void nwe_destroy(nwe_ctx *ctx);

/* Message of the last failed call on `ctx` (or of the last failed nwe_create when ctx == NULL). */
const char *nwe_last_error(const nwe_ctx *ctx);

/* Upload one NeRFModel (nerf/models/nerf_model.py:10-43, use_view_dirs=True) from HOST fp32 tensors in
 * PyTorch nn.Linear layout ([out,in] row-major, y = x W^T + b).  Copied and repacked inside; the caller
 * may free its buffers on return.  Replaces load_state_dict + .cuda() (handler.py:106-141).
 *   depth, width   D, W of the density trunk
 *   in_xyz,in_dir  encoded input widths (63, 27): 3 + 6*num_freqs
 *   skip_layer     i such that gamma(x) is concatenated in front of h AFTER layer i's ReLU
 *                  (nerf_model.py:58-59; 4 for D=8), or -1
 *   w, b           depth+4 pointers each, ordered: _pts_linears[0..depth-1], _views_linears[0],
 *                  _feature_linear, _alpha_linear, _rgb_linear
 * Domain: depth 1..16, even width 2..256, in_xyz = 3 + 6 k <= 93, in_dir = 3 + 6 k <= 63 (NWE_ERR_UNSUPPORTED outside; a
 * refused call leaves the network set before it in place); a skip_layer that feeds no layer (outside 0..depth-2) is no skip.
 * The coarse and the fine network SHARE THEIR ENCODINGS, as in the reference, where one Embedding per input serves both
 * (handler.py:93-103): with n_importance > 0 a render of two networks that differ in in_xyz or in_dir is refused with
 * NWE_ERR_STATE (the kernels encode a ray's view direction once, for both passes).  Under NWE_PREC_F32 the two may differ in
 * depth, width and skip (net_depth_fine / net_width_fine, handler.py:42-45,106-119); the MFMA precisions need one shape. */
int nwe_set_network(nwe_ctx *ctx, int which, int depth, int width, int in_xyz, int in_dir, int skip_layer,
                    const float *const *w, const float *const *b);

/* The same for NeRFModel(use_view_dirs=False) (nerf/models/nerf_model.py:41-43,82-83; the handler builds it with
 * input_ch_views = 0 and output_ch = 5, handler.py:97-119): the trunk and ONE output layer.  w, b: depth+1 pointers each,
 * _pts_linears[0..depth-1] then _output_linear [output_ch, width]; output_ch >= 4, channels 0..2 are rgb_raw and channel 3
 * sigma_raw (model_utils.py:62,71), further channels are ignored as the reference ignores them.  Such networks render with
 * every precision where the shape is one the MFMA kernel is instantiated for (widths 128 and 256, depth 6 or 8 with the skip
 * after layer 4, or depth 4 without) - it evaluates the trunk and
 * then one tile of _output_linear - and with NWE_PREC_F32 otherwise; they take 8-column rays in nwe_render_rays ([o d near far], nerf/rays/rays.py:26-30
 * without the view directions) and both networks of a context must be of the same kind. */
int nwe_set_network_no_view_dirs(nwe_ctx *ctx, int which, int depth, int width, int in_xyz, int skip_layer, int output_ch,
                                 const float *const *w, const float *const *b);

/* Sampling tables computed by the host with torch.linspace (its bits are not i/(n-1)):
 *   t_vals[n_samples] = linspace(0,1,Ns) and one_minus_t[n_samples] = 1 - t_vals  (handler.py:216-218)
 *   u[n_importance]   = linspace(0,1,Ni)                                        (nerf/rays/rays.py:95)
 * n_importance may be 0 (coarse only; u may then be NULL).  n_samples 2..128 and n_importance 0..256 (NWE_ERR_UNSUPPORTED
 * outside); importance samples need n_samples >= 3, since sample_pdf takes weights[..., 1:-1] (NWE_ERR_INVALID).
 * nwe_render is asynchronous, so this call and nwe_set_network[_no_view_dirs] first wait for every launch of this context
 * that is still in flight, on whatever stream, before they touch the device tables and weights those launches read: the
 * caller need not synchronise before reconfiguring.  (nwe_set_white_background and the other host-side switches are copied
 * at launch and never reach a launch already queued.) */
int nwe_set_sampling(nwe_ctx *ctx, const float *t_vals, const float *one_minus_t, int n_samples,
                     const float *u, int n_importance);

/* Render rays [row_begin,row_end) x [0,W) of n_poses pinhole views.  c2w: HOST, n_poses*16 floats,
 * row-major 4x4 camera-to-world.  Output ray index = (p*(row_end-row_begin) + (h-row_begin))*W + w.
 * Ray generation follows nerf/rays/rays.py:6-71; the render loop nerf_replica_inference_handler.py:203-277.
 * Asynchronous on `stream` (a hipStream_t, NULL = default stream) when c2w is pageable host memory (the poses are
 * staged before the call returns); a pinned c2w must stay valid until the stream has passed the call.  A context may
 * have launches in flight on several streams (each launch owns its pose table); it is still not thread-safe, and with
 * more than four launches queued the call blocks until the oldest has finished.
 * Replaces: create_rays + rays.cuda() + _render_rays of render_coordinates (handler.py:172-177). */
int nwe_render(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy,
               float near, float far, int row_begin, int row_end, int precision, const nwe_outputs *out,
               void *stream);

/* One process, several contexts: every context renders one contiguous row tile of every pose - context i the rows
 * dist.shard_rows(H, n_ctx)[i], the first H % n_ctx tiles one row longer - on a stream of its own, and copies it into the
 * caller's row-major frames on contexts[0]'s device (hipMemcpyPeerAsync: xGMI between devices, a plain device copy when the
 * contexts share a device; "several tiles on one device" and "one tile per device" are the same code).  The caller's
 * stream (on contexts[0]'s device) continues when all tiles have landed.  Every context must have its networks and
 * sampling tables set, identically.  rgb_dev [n_poses,H,W,3], depth_dev / acc_dev [n_poses,H,W], flags_dev [1]; each may be
 * NULL.  Errors are reported on contexts[0].
 * Why it exists: the reference renders from its GUI thread (application/app.py:336 -> application/workspace.py:66 ->
 * render_coordinates), which cannot be one rank of a torchrun job; this is the multi-GPU path of that call.  (One process
 * per GPU with an RCCL gather is nwe_amd/dist.py.) */
int nwe_render_tiled(nwe_ctx *const *contexts, int n_ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy,
                     float cx, float cy, float near, float far, int precision, float *rgb_dev, float *depth_dev,
                     float *acc_dev, uint32_t *flags_dev, void *stream);

/* What the last nwe_render_tiled on contexts[0] went through without failing but the caller should know (peer access
 * between two devices not available or not enabled: the tile copies are then staged by the runtime); "" if nothing. */
const char *nwe_last_warning(const nwe_ctx *ctx);
/* How `tile`'s device reaches `first`'s (contexts[0]'s) memory in nwe_render_tiled: 1 direct (same device, or peer access
 * over xGMI enabled), 0 hipDeviceCanAccessPeer says no (staged copies), -1 the query or hipDeviceEnablePeerAccess failed. */
int nwe_debug_peer_access(const nwe_ctx *first, const nwe_ctx *tile);

/* Generate the rays of nwe_render() without rendering them: DEVICE rays_out [n_poses*(row_end-row_begin)*W, 11]
 * fp32 = [o(3) d(3) near far viewdir(3)], bit-identical to the reference's CPU result.
 * Replaces: create_rays (nerf/rays/rays.py:6-32). */
int nwe_create_rays(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy,
                    float near, float far, int row_begin, int row_end, float *rays_out_dev, void *stream);

/* Render precomputed rays: DEVICE [n_rays,11] fp32 = [o(3) d(3) near far viewdir(3)] (rays.py:26-30); [n_rays,8] without the
 * view directions when the context's networks were set with nwe_set_network_no_view_dirs.
 * Precondition: near <= far on every ray (see "near <= far" above).
 * Replaces: NeRFReplicaInferenceHandler._render_rays(flat_rays) (handler.py:187-201). */
int nwe_render_rays(nwe_ctx *ctx, const float *rays_dev, int64_t n_rays, int precision, const nwe_outputs *out,
                    void *stream);

/* Device outputs of nwe_query_points, owned by the caller; raw or sigma may be NULL, not both. */
typedef struct nwe_point_outputs {
    uint64_t struct_bytes;  /* = sizeof(nwe_point_outputs), checked like nwe_outputs.struct_bytes */
    float *raw;             /* [n_points,4]  [rgb_raw(3), sigma_raw]: run_network's row, no sigmoid, no ReLU */
    float *sigma;           /* [n_points]    sigma_raw alone */
    uint32_t *flags;        /* [1]  NWE_FLAG_RAW OR-ed in when a value written is NaN or inf (caller zeroes it) */
} nwe_point_outputs;

/* The point query: network `which` at arbitrary points, on the kernels that render.
 * Replaces: run_network (nerf/models/model_utils.py:13-30): points [N,S,3] and view directions [N,3] give the raw network
 * output [N,S,4] (the `show_endpoint` feature columns are not produced).
 *   points_dev      DEVICE [n_points,3] fp32 world coordinates; the kernel divides by 10 itself, as everywhere
 *                   (handler.py:93).
 *   dirs_dev        DEVICE [ceil(n_points / points_per_dir),3]: point i is evaluated with direction i / points_per_dir.
 *                   The reference's viewdirs[:, None].expand(inputs.shape) is points_per_dir = S; 1 = a direction per point.
 *                   Used as given, not normalised, like the view-direction columns of nwe_render_rays (handler.py:210-214).
 *                   NULL: required for a network set with nwe_set_network_no_view_dirs (a pointer there is NWE_ERR_INVALID);
 *                   accepted for a network with view directions only when out->raw is NULL - sigma does not depend on the
 *                   direction.
 *   out             raw and / or sigma.  With out->raw == NULL, a direction given or not, the MFMA kernels evaluate the
 *                   density trunk only where the shape has that path (the folded formulation except 6-deep networks with
 *                   the skip after layer 4) and the full network with the colour dropped elsewhere; sigma has the same bits
 *                   either way, and the bits of raw[.., 3].
 * Every output row depends on its point and its direction and on nothing else: not on n_points, the rows around it, its
 * place in a workgroup, nwe_debug_set_query_steps, the stream, or which outputs were requested.  It is, bit for bit, what
 * nwe_render_rays writes to raw_coarse for a sample that sits at that point (o = p, near = far = 0) with that view direction.
 * Needs network `which` set and nothing else: no nwe_set_sampling, no second network, and no rule about the other network's
 * shape - a context that holds a 4x128 coarse and an 8x256 fine network answers queries to both under the MFMA precisions.
 * Ignores white background, early termination, shared coarse pass, separate passes, decomposition and work queue.  Neither
 * uses nor clears the one-shot hooks and training tables, and moves none of nwe_last_kernel_ms, nwe_last_launch_parts,
 * nwe_debug_last_plan, nwe_last_ray_evaluations, nwe_debug_last_queue: its launches have events of their own.
 * Refuses, in this order and before anything is queued: NULL or host-only context (NWE_ERR_STATE); NULL out, wrong
 * struct_bytes, which not 0 / 1, n_points < 0 or >= 2^31, points_per_dir < 1, NULL points_dev with n_points > 0, neither raw
 * nor sigma (NWE_ERR_INVALID); unknown precision (NWE_ERR_INVALID); network not set (NWE_ERR_STATE); the dirs_dev rules
 * (NWE_ERR_INVALID); an MFMA precision for a shape without an MFMA kernel (NWE_ERR_UNSUPPORTED, "use NWE_PREC_F32").
 * n_points == 0 is NWE_OK: nothing is launched and nwe_last_query_ms does not change.
 * Asynchronous on `stream`.  Query launches have an event ring of their own (four launches in flight; a fifth call waits for
 * the oldest), which the wait of nwe_set_network / nwe_set_sampling covers on whatever streams they are: weights a query
 * still reads are never repacked under it.
 * Non-finite and out-of-range coordinates follow the render path's rule above: never a finite wrong value under
 * NWE_PREC_F16X3 / F16X1 (NaN, and NWE_FLAG_RAW), every finite coordinate defined under NWE_PREC_F32. */
int nwe_query_points(nwe_ctx *ctx, int which, const float *points_dev, int64_t n_points, const float *dirs_dev,
                     int64_t points_per_dir, int precision, const nwe_point_outputs *out, void *stream);
/* Time of the most recent query launch, from HIP events of its own (like nwe_create_rays, it is no render launch); blocks
 * until it has finished; < 0 if there was none yet. */
float nwe_last_query_ms(nwe_ctx *ctx);
/* Test hook: the packets (128 points under the MFMA precisions, 16 under NWE_PREC_F32) a query workgroup walks, 1..256;
 * 0 = automatic (the default): packets / (8 x the device's CUs), at least 1 and at most 256.  Results do not depend on it. */
int nwe_debug_set_query_steps(nwe_ctx *ctx, int steps);

/* uint8 = (255 * clip(x,0,1)) truncated, elementwise over n floats on the device.
 * Replaces: to8b_np (nerf/models/model_utils.py:9) of render_coordinates' tail (handler.py:183). */
int nwe_to8b(nwe_ctx *ctx, const float *rgb_dev, uint8_t *out_dev, int64_t n, void *stream);

/* Algorithmic FLOPs (2 x GEMM MACs of the reference formulation) of one MLP evaluation of network `which`. */
int64_t nwe_flops_per_eval(const nwe_ctx *ctx, int which);

/* Time of the most recent RENDER launch on this context (nwe_render / nwe_render_rays / this context's tile of
 * nwe_render_tiled), from HIP events recorded on its stream around the kernel; blocks until that launch has finished.
 * nwe_create_rays does not count, however often it is called (it has events of its own), and neither does a call that was
 * refused, zero rays, or a launch refused after its argument checks ("coarse and fine networks must have the same
 * shape"): this call and nwe_last_launch_parts then still describe the last launch that was made.  Returns < 0 if nothing
 * was launched.  Like every entry point it leaves the calling
 * thread's current HIP device as it found it.
 * A time is read from the launch's events once and kept: this call, nwe_last_launch_parts, nwe_last_coarse_launch,
 * nwe_last_query_ms, nwe_last_grid_ms and nwe_last_sparse_ms return the same float, exactly, for as long as they describe
 * the same launch, however often they are asked and whatever is launched in between. */
float nwe_last_kernel_ms(nwe_ctx *ctx);

/* The same launch taken apart: a frame whose last round of workgroups is ragged is rendered as TWO launches of the kernel
 * template back to back (the full rounds as four-packet workgroups, the rest sample-split; nwe_debug_last_plan == 2).
 * ms2[0], rays2[0]: the first (or only) launch; ms2[1], rays2[1]: the second, -1 / 0 if there was none.  Blocks like
 * nwe_last_kernel_ms.  With the work queue on (nwe_debug_set_work_queue, the default for frames larger than the device) the
 * second launch runs BESIDE the first: ms2[1] is then how long the frame ran beyond its first launch, not the second kernel's
 * time, often next to nothing: a rate computed from it means nothing.  On the tail path (nwe_debug_set_work_queue) the first launch
 * renders the second's rays as well: ms2[0] is the whole frame, ms2[1] an empty launch, rays2 the plan's split all the same.  The parts are positive (never 0: a part below the
 * timer's step of 1e-5 ms is reported as that step) and add up to nwe_last_kernel_ms to within that step. */
int nwe_last_launch_parts(nwe_ctx *ctx, float *ms2, int64_t *rays2);

/* --- test hooks ------------------------------------------------------------------------------- */

/* Size in bytes / host copy of the MFMA weight stream packed for network `which` (0 if that network
 * has no MFMA kernel).  Layout: see DESIGN.md "weight stream".  Works on host-only contexts. */
int64_t nwe_packed_bytes(const nwe_ctx *ctx, int which);
int nwe_packed_copy(const nwe_ctx *ctx, int which, void *host_dst, int64_t bytes);
/* The rest of the packed network: the per-chunk bias table (32 floats per chunk) and the power of two the packed
 * weights are multiplied by. */
int64_t nwe_packed_bias_count(const nwe_ctx *ctx, int which);
int nwe_packed_bias_copy(const nwe_ctx *ctx, int which, float *host_dst, int64_t count);
float nwe_packed_scale(const nwe_ctx *ctx, int which);
/* 1 if every value the colour layers of network `which` hold as packed for the MFMA kernels is finite (the folded view layer
 * formed in fp64 with its view-direction columns, the rgb head, both biases), 0 if not or if the network is not packed folded,
 * -1 if it has not been set.  Decided once per nwe_set_network; no device needed.  See nwe_debug_set_colour_skip. */
int nwe_packed_colour_finite(const nwe_ctx *ctx, int which);

/* Test hook: the NEXT nwe_render_rays call takes the fine-pass sample depths from z_dev (DEVICE [n_rays, S],
 * sorted per ray) instead of its own importance sampling; cleared after that call.  Lets a test feed the
 * reference's own depths and compare the fine pass alone.
 * This holds for every one-shot hook below and for nwe_set_train_tables: "that call" is the next nwe_render_rays whatever
 * becomes of it.  A refused call consumes the hooks too (unsupported precision or shape, bad arguments, a wrong
 * struct_bytes), and so does a call with zero rays: no hook survives into a call whose caller did not set it.  nwe_render
 * and nwe_render_tiled neither use nor clear the hooks; NULL pointers disarm them. */
int nwe_debug_set_fine_depths(nwe_ctx *ctx, const float *z_dev);

/* Test hooks in the same style (the NEXT nwe_render_rays call, cleared after it); both kernels honour them:
 *   nwe_debug_set_raw             network outputs from the caller instead of evaluating the MLP: DEVICE raw_coarse
 *                                 [n_rays, n_samples, 4] and / or raw_fine [n_rays, S, 4] (either may be NULL), so that
 *                                 compositing (nerf/models/model_utils.py:49-100) is checked on the reference's own
 *                                 edge vectors (sigma <= 0 everywhere, saturated alpha, sigma_last = +-1e-11);
 *   nwe_debug_set_coarse_weights  coarse weights [n_rays, n_samples] from the caller instead of running the coarse pass
 *                                 (its outputs are then not written), so that the inverse-CDF sampling
 *                                 (nerf/rays/rays.py:74-121) is checked on given weights. */
int nwe_debug_set_raw(nwe_ctx *ctx, const float *raw_coarse_dev, const float *raw_fine_dev);
int nwe_debug_set_coarse_weights(nwe_ctx *ctx, const float *weights_dev);

/* Test hook: networks uploaded AFTER this call are packed for the MFMA kernel with (1, the default) or without (0)
 * _feature_linear multiplied into _views_linears (nerf/models/nerf_model.py:64-70: the feature layer has no activation,
 * so W_v [W_f h + b_f; gamma(d)] + b_v = (W_v[:, :W] W_f) h + ...; fp64 product on the host).  0 evaluates the feature
 * layer as the reference formulates it (8x256 and 4x128 only); kept for one-to-one comparison. */
int nwe_debug_set_fold(nwe_ctx *ctx, int on);

/* rendering.white_background of the reference's YAML (nerf/models/model_utils.py:97-98): when on, every rgb output
 * (coarse and fine) is rgb + (1 - acc).  Off by default, as in all four office configs. */
int nwe_set_white_background(nwe_ctx *ctx, int on);

/* Early ray termination, opt-in: min_transmittance = eps, 0 <= eps < 1; 0 (the default) is off and changes nothing.  NaN,
 * a negative value or eps >= 1 is NWE_ERR_INVALID and the previous value stays.  Host-side like nwe_set_white_background:
 * copied at launch, works on a host-only context; nwe_get_early_termination returns the value (-1 for a NULL context).
 * The rule is per ray: the outputs of a ray do not depend on which rays share its workgroup.  In the TERMINATED PASS - the
 * pass that produces the frame's outputs: the fine pass when n_importance > 0, the only pass otherwise - sample i of a ray
 * contributes nothing (w_i = 0) when its transmittance T_i is below eps.  T_i is the reference's trans[:, i]
 * (nerf/models/model_utils.py:79-80), the fp32 value alpha_i is multiplied by; it runs on unmasked.  In reference terms the
 * result is raw2outputs with weights * (trans >= eps).  Everything else is as without it: the 1e10 last interval,
 * white_background (rgb + 1 - acc with the masked acc), the flags.  A NaN T_i is not below eps, so a ray with NaN keeps the
 * reference's NaN pattern.  The coarse pass of a frame with importance sampling is never touched: its weights feed
 * sample_pdf, which amplifies the smallest change.
 * Error bound, by construction: on the supported domain (near <= far, so alpha in [0, 1]) T never increases, so a masked ray
 * stays masked and the dropped weights sum to less than eps: |d rgb| < eps per channel, |d acc| < eps, |d depth| < eps * z_last.
 * The skip is a pure optimisation under that rule: a workgroup stops evaluating the pass once every ray it owns is masked
 * (up to one iteration late, nwe_mfma_render.h); a ray masked before its group is done has its later samples evaluated and
 * ignored.  Results are bit-identical across the work decompositions, the hybrid plan, row tiles, pose batches and the
 * tiles of nwe_render_tiled, as without it.
 * Honoured by calls that request nothing but rgb / depth / acc / flags of pinhole views - nwe_render and nwe_render_tiled - in
 * all three precisions.  With eps > 0 every other call is refused with NWE_ERR_UNSUPPORTED and a message that names the
 * setting, behind every refusal the call has without it: any further output (per-sample and coarse outputs have no meaning
 * past a stop), all of nwe_render_rays with or without hooks or training tables, and under the MFMA precisions a network
 * packed unfolded (nwe_debug_set_fold(0)) or a shape whose terminating kernel was not built (NWE_PREC_F32 renders both). */
int nwe_set_early_termination(nwe_ctx *ctx, float min_transmittance);
float nwe_get_early_termination(const nwe_ctx *ctx);

/* A coarse pass shared by k x k pixel blocks, opt-in: k = 1..16; 1 (the default) is off and changes nothing.  Anything else is
 * NWE_ERR_INVALID and the previous value stays.  Host-side like nwe_set_white_background: copied at launch, works on a
 * host-only context; nwe_get_shared_coarse returns the value (-1 for a NULL context).
 * Why: a frame that asks for rgb / depth / acc reads nothing of its coarse pass but the weights that feed sample_pdf.  Near and
 * far are the frame's, so the coarse depths and z_mid are the same for every ray and only the weights differ from ray to ray,
 * smoothly in the pixel.  With k > 1 one ray per block runs the coarse pass and the block's pixels draw their importance
 * samples from its weights: 1 - 1/k^2 of the coarse evaluations of an aligned frame go.  It is an approximation.
 * The rule, for nwe_render / nwe_render_tiled with n_importance > 0:
 *   - pixel (h, w) of pose p belongs to block (h / k, w / k) of the WHOLE image, not of the rows of the call;
 *   - the block's representative pixel is (min(k (h / k) + k / 2, H - 1), min(k (w / k) + k / 2, W - 1));
 *   - ray r takes the coarse weights of its representative ray rep(r) of the same pose: in reference terms
 *     sample_pdf(z_mid, weights[rep][..., 1:-1], ...) at nerf_replica_inference_handler.py:237, and since z_vals are the
 *     frame's, z_fine[r] == z_fine_full[rep(r)], the depths an ordinary frame gives the representative;
 *   - everything behind that is the ray's own: its points, its view direction, the fine network, the compositing.
 * Blocks sit on the absolute pixel grid, so a pixel's outputs depend on nothing but the frame: row tiles (whose
 * representatives may lie outside their rows), pose batches, the work decompositions, the hybrid plan and the tiles of
 * nwe_render_tiled stay bit-identical to one another, as without it.
 * With n_importance == 0 there is no pass to share and the call renders exactly as with k = 1.
 * No ray has a coarse pass of its own then, so the coarse flag bits (NWE_FLAG_*_COARSE) are never raised; the representatives'
 * coarse pass writes nothing but the weights.
 * A call is two launches on the caller's stream: a producer over the representatives of the blocks its rows touch, which
 * writes their weights to a table the launch owns, and behind it a consumer over the call's rays.
 * With k > 1 every other call is refused with NWE_ERR_UNSUPPORTED and a message that names the setting, behind every refusal
 * the call has without it and whatever n_importance is: any output beyond rgb / depth / acc / flags, all of nwe_render_rays (no
 * pixel grid), under the MFMA precisions a network packed unfolded (nwe_debug_set_fold(0); NWE_PREC_F32 renders it), and
 * every call while early termination is on as well (min_transmittance > 0: the combination is not built). */
int nwe_set_shared_coarse(nwe_ctx *ctx, int k);
int nwe_get_shared_coarse(const nwe_ctx *ctx);

/* Separate passes, opt-in: on = 0 or 1; 0 (the default) is off and changes nothing.  Anything else is NWE_ERR_INVALID and the
 * previous value stays.  Host-side like nwe_set_white_background: copied at launch, works on a host-only context;
 * nwe_get_separate_passes returns the value (-1 for a NULL context).
 * Why: the fused MFMA kernel runs both passes with the instantiation of ONE network shape, so a small coarse network under a
 * full fine one (net_depth / net_width against net_depth_fine / net_width_fine of the reference's YAML) is refused by the MFMA
 * precisions although each shape has kernels.  With the mode on, a call with n_importance > 0 under NWE_PREC_F16X3 / F16X1 is
 * two launches on the caller's stream: a coarse launch over the call's rays with the kernels of the coarse network's shape,
 * which writes every sample's weight to a table the launch owns (or to weights_coarse, if the caller asked for it), and behind
 * it a fine launch with the kernels of the fine network's shape, which reads the table where the fused kernel runs its coarse
 * pass.  The two networks may differ in depth, width and skip; each shape must have an MFMA instantiation, and both must agree
 * in their encodings and in their formulation (view directions or none; packed folded or not), else the call is refused by name.
 * It is exact: the table carries the floats the fused kernel keeps on chip between its passes, and each launch computes what
 * the fused kernel's pass computes.  With two networks of one shape every output of every call is bit-identical to the same
 * call with the mode off; with two shapes the coarse outputs are those of a (coarse, coarse) context and the others those of a
 * (fine, fine) context fed these weights through nwe_debug_set_coarse_weights, bit for bit.  Work decompositions, the hybrid
 * plan, row tiles, pose batches and the tiles of nwe_render_tiled stay bit-identical to one another.
 * Every call that renders with the mode off renders with it on: nwe_render and nwe_render_tiled with any outputs,
 * nwe_render_rays, its one-shot hooks and its training tables.  Coarse outputs (raw_coarse, weights_coarse, rgb_coarse /
 * depth_coarse / acc_coarse / disp_coarse) come from the coarse launch, everything else from the fine launch; *flags is the OR
 * of both.  A call armed with nwe_debug_set_coarse_weights has no coarse launch.  A call that requests nothing but rgb / depth /
 * acc / flags of pinhole views takes the lean kernels of the shared coarse pass, each pixel its own representative: its coarse
 * launch writes nothing but the weights and raises the coarse flag bits the fused call raises (NWE_FLAG_RGB_COARSE under the
 * rule above).
 * With n_importance == 0 there is one pass and the call renders as with the mode off.  NWE_PREC_F32 ignores the mode: the fp32
 * kernel takes two shapes in one launch.
 * With the shared coarse pass (nwe_set_shared_coarse, k > 1) the two compose - that call already is these two launches: the
 * producer takes the coarse network's kernels and the consumer the fine network's, under the shared coarse pass's own rules.
 * Refused with NWE_ERR_UNSUPPORTED and a message that names the setting, behind every refusal the call has without it, under
 * the MFMA precisions: every call while early termination is on (min_transmittance > 0: terminating consumer kernels are not
 * built), and two networks of which only one was packed unfolded (nwe_debug_set_fold).
 * Timing: nwe_last_kernel_ms spans both launches, nwe_last_coarse_launch gives the coarse launch's time and ray count,
 * nwe_last_launch_parts and nwe_debug_last_plan describe the fine launch (each launch picks its own plan;
 * nwe_debug_set_decomposition forces both), nwe_last_ray_evaluations reports executed == full.  The table is
 * n_rays * n_samples floats per launch in flight (164 MB for an 800 x 800 x 64 frame); if it cannot be allocated the call fails
 * with NWE_ERR_HIP, nothing is launched and the timing calls keep describing the last launch that was made. */
int nwe_set_separate_passes(nwe_ctx *ctx, int on);
int nwe_get_separate_passes(const nwe_ctx *ctx);

/* Occupancy grid, opt-in: a context may hold ONE grid; none (the default) changes nothing.  A grid is an axis-aligned box
 * lo[3] < hi[3] in world coordinates, a resolution res = (rx, ry, rz) and rx * ry * rz bits, 1 = occupied: each axis 1..1024,
 * fewer than 2^31 cells in all; bit (ix * ry + iy) * rz + iz sits in word >> 5 at bit & 31 (the layout of a [rx, ry, rz]
 * array, z fastest).
 * The rule, per sample and in BOTH passes:
 *   - the point is the fp32 point the kernels encode: o + d * z, multiply then add (handler.py:223 / :246), before the
 *     division by 10;
 *   - its cell is floorf((p_c - lo_c) * inv_c) per axis, a plain fp32 subtraction and multiplication, with
 *     inv_c = (float)r_c / (hi_c - lo_c) formed once on the host in fp32 (nwe_get_occupancy reports it);
 *   - a point that is not finite, or whose cell index is outside 0 .. r_c - 1 on any axis, is OCCUPIED: outside the box
 *     everything is evaluated;
 *   - a sample in an empty cell has raw = (0, 0, 0, 0) in place of the network's output: in reference terms run_network's rows
 *     (nerf/models/model_utils.py:13-30) are replaced before raw2outputs, in the coarse pass - so its weight feeding sample_pdf
 *     is 0 - and in the fine pass alike.  All four channels, not only sigma: the result of a ray then depends on nothing but
 *     the ray and the grid, never on which rays share its workgroup, and a non-finite colour under a zero weight cannot leak.
 * The skip is a pure optimisation under that rule: a workgroup does not evaluate a sample iteration in which every live ray
 * it owns is in an empty cell (the sample-split plan: all four samples of the iteration); in a mixed iteration the network
 * runs and the masked rays' outputs are replaced.  Frames stay bit-identical across the two work decompositions, the hybrid
 * plan, row tiles, pose batches and the tiles of nwe_render_tiled, as without a grid.  Two identities follow:
 *   - a grid with every bit set renders the bits of the same call without a grid;
 *   - a grid is EXACT for a network whose sigma_raw is <= 0 and finite, with finite colours, throughout every cell marked
 *     empty: it renders, bit for bit, what the same call renders without one.
 * Anything else is an approximation whose size is the grid's own error: density the grid calls empty is not rendered.
 * Honoured by calls that request nothing but rgb / depth / acc / flags of pinhole views - nwe_render and nwe_render_tiled - in
 * all three precisions, for the folded and the no-view-dirs formulations, with or without importance samples.  While a grid
 * is set every other call is refused with NWE_ERR_UNSUPPORTED and a message that names the setting, behind every refusal the
 * call has without it: any further output, all of nwe_render_rays with its hooks and training tables, under the MFMA
 * precisions a network packed unfolded (nwe_debug_set_fold(0)) or a shape whose occupancy kernel was not built (NWE_PREC_F32
 * renders both), and every call while early termination (min_transmittance > 0), a shared coarse pass (k > 1) or separate
 * passes are on as well: these combinations are not built.  nwe_query_points ignores the grid.
 * nwe_set_network and nwe_set_network_no_view_dirs CLEAR the grid - a grid describes the networks it was made for; a refused
 * one leaves it in place, like the network.  The grid calls below wait for this context's launches in flight, like
 * nwe_set_sampling.
 * nwe_last_ray_evaluations: out[0] = for every group of rays, its live rays x the samples of the iterations it evaluated, both
 * passes.  A group is 128 consecutive rays of a launch (packets), 32 (sample split: an iteration is four samples), or - under
 * NWE_PREC_F32 - 16 consecutive rays of the call; nwe_last_launch_parts says which rays went to which launch.
 *   nwe_set_occupancy    copies the words ((rx ry rz + 31) / 32 of them, from the host or - bits_on_device != 0 - the context's
 *                        device) into a buffer the context owns.  Refused by name (NWE_ERR_INVALID): null pointers, a box that
 *                        is not finite or not lo < hi on every axis, a resolution outside the domain.
 *   nwe_clear_occupancy  no grid.
 *   nwe_get_occupancy    the grid's box, resolution, the fp32 inv the kernels multiply by and the number of occupied cells; any
 *                        pointer may be null.  NWE_ERR_STATE (and nothing written) when no grid is set.
 *   nwe_occupancy_copy   the words, n_words = (rx ry rz + 31) / 32; bits behind the last cell are 0.
 * Set, clear, get and copy work on a host-only context (the bits are kept on the host there).
 *   nwe_build_occupancy  builds the grid from the networks that are set, on the device: per cell a probes^3 lattice of points,
 *                        probes 1..4, along an axis at ((float)i + ((float)j + 0.5f) / probes) * step + lo for cell i and probe j,
 *                        step = (float)(((double)hi - (double)lo) / r), every operation rounded to fp32 on its own (probes = 1:
 *                        the cell's centre); sigma_raw of EVERY set network there, by the sigma-only path of nwe_query_points
 *                        in `precision`; a cell is occupied if any value is > threshold or not finite; then `dilate` (0..2)
 *                        steps of dilation with the 3 x 3 x 3 box.  The probes are evaluated in chunks through a scratch buffer
 *                        the context keeps.  Synchronous: queued on `stream` and waited for.  Refused: a host-only context,
 *                        no network set (NWE_ERR_STATE); the box and resolution as above, probes, dilate, a NaN threshold,
 *                        an unknown precision (NWE_ERR_INVALID); an MFMA precision for a shape without a query kernel
 *                        (NWE_ERR_UNSUPPORTED, the query's own message). */
int nwe_set_occupancy(nwe_ctx *ctx, const float *lo, const float *hi, const int *res, const uint32_t *bits, int bits_on_device);
int nwe_clear_occupancy(nwe_ctx *ctx);
int nwe_get_occupancy(const nwe_ctx *ctx, float *lo, float *hi, int *res, float *inv, int64_t *occupied_cells);
int nwe_occupancy_copy(const nwe_ctx *ctx, uint32_t *host_words, int64_t n_words);
int nwe_build_occupancy(nwe_ctx *ctx, const float *lo, const float *hi, const int *res, int probes, float threshold, int dilate,
                        int precision, void *stream);

/* Baked coarse pass, opt-in: a context may hold ONE coarse density grid; none (the default) changes nothing.  A grid is an
 * axis-aligned box lo[3] < hi[3] in world coordinates, a resolution res = (rx, ry, rz), each axis 1..512, and rx * ry * rz fp32
 * values of sigma_raw (before the ReLU) at the cell centres, in the layout of a [rx, ry, rz] array, z fastest - what
 * handler.density_grid returns.
 * Why: a lean frame reads nothing of its coarse pass but the weights that feed sample_pdf, and the quantity behind them,
 * sigma_coarse(x), depends on the position only.  While a grid is set, a lean call with n_importance > 0 - nwe_render or
 * nwe_render_tiled requesting nothing but rgb / depth / acc / flags of pinhole views - does not run the coarse network.
 * The rule, for each ray and each coarse sample i:
 *   - the depth z_i and the fp32 point p = o + d * z_i are the ones the kernels encode (near * (1 - t) + far * t, handler.py:218;
 *     multiply then add, handler.py:223), before the division by 10;
 *   - its grid coordinate is g_c = (p_c - lo_c) * inv_c - 0.5f per axis: an fp32 subtraction, multiplication and subtraction, each
 *     rounded on its own, with inv_c = (float)r_c / (hi_c - lo_c) formed once on the host in fp32 (nwe_get_coarse_grid reports it);
 *   - OUTSIDE the box the sample has sigma_raw = 0: if any p_c is not finite, or g_c < -0.5f or g_c > r_c - 0.5f on any axis.
 *     Nothing is known there; the weight is 0 and only sample_pdf's 1e-5 floor remains;
 *   - inside, i0 = floorf(g_c) and f_c = g_c - i0 (exact); the two indices i0 and i0 + 1 are clamped to 0 .. r_c - 1, so within half
 *     a cell of a face the value is the face cell's; the eight values are interpolated along z, then y, then x, each
 *     interpolation a + (b - a) * f in three separately rounded fp32 operations, no FMA: a numpy float32 restatement gives the
 *     same bits (tests/coarse_grid.py).  A non-finite grid value propagates;
 *   - the ray's coarse weights are raw2outputs' fourth return value (nerf/models/model_utils.py:49-100) for
 *     raw = (0, 0, 0, sigma_raw_i), computed with the device code the render kernels composite with: for equal sigma they are,
 *     bit for bit, the weights a coarse pass produces;
 *   - everything behind that is the ordinary call: sample_pdf on weights[1:-1], the merge, the fine network, the compositing.
 * So a ray's outputs depend on the ray and the grid only; frames stay bit-identical across the work decompositions, the hybrid
 * plan, row tiles, pose batches and the tiles of nwe_render_tiled; the coarse flag bits are never raised.  With
 * n_importance == 0 the only pass is the output and the call renders exactly as without a grid.
 * It is an approximation whose size is the trilinear interpolation error of the coarse density at the grid's resolution.
 * A call is two launches on the caller's stream: the producer (one thread per ray; it fills the slot's weight table
 * [n_samples][n_rays] from the grid) and behind it the consumer of the shared coarse pass at k = 1 with the FINE network's
 * kernels.  The coarse network's shape is therefore not constrained; under the MFMA precisions the fine network's shape needs
 * its sharing kernels.  nwe_debug_plan reports the coarse stage as active, role 1 (producer), n_rays = the call's rays,
 * n_launches = 1 and variant = plan = -1: it is no MFMA launch group and has neither; the rest of the stage is zero.
 * nwe_last_ray_evaluations: out[1] stays n_rays * (2 n_samples + n_importance), out[0] = n_rays * (n_samples + n_importance).
 * nwe_last_coarse_launch: the producer's time and the call's rays; nwe_last_kernel_ms spans both launches.
 * While a grid is set every other call is refused with NWE_ERR_UNSUPPORTED and a message that names the setting, behind every
 * refusal the call has without it and whatever n_importance is: any output beyond rgb / depth / acc / flags, all of
 * nwe_render_rays with its hooks and training tables, under the MFMA precisions (n_importance > 0) a fine network packed unfolded
 * (nwe_debug_set_fold(0)) or one whose sharing kernels were not built (NWE_PREC_F32 renders both), a stamped launch, and every
 * call while early termination (min_transmittance > 0), a shared coarse pass (k > 1), separate passes or an occupancy grid is on
 * as well: these combinations are not built.  nwe_query_points ignores the grid.
 * nwe_set_network / nwe_set_network_no_view_dirs with which == NWE_NET_COARSE CLEAR the grid - it describes that network; setting
 * the fine network leaves it, and so does a refused call.  The grid calls below wait for this context's launches in flight,
 * like nwe_set_sampling.
 *   nwe_set_coarse_grid      copies the values (from the host or - on_device != 0 - the context's device) into a buffer the
 *                            context owns; a host-only context keeps them on the host.  Refused by name (NWE_ERR_INVALID): null
 *                            pointers, a box that is not finite or not lo < hi on every axis (or so thin that inv is not finite),
 *                            a resolution outside the domain.
 *   nwe_clear_coarse_grid    no grid.
 *   nwe_get_coarse_grid      the grid's box, resolution and the fp32 inv the kernel multiplies by; any pointer may be null.
 *                            NWE_ERR_STATE (and nothing written) when no grid is set.
 *   nwe_coarse_grid_copy     the values, n_values = rx * ry * rz, to the host.
 *   nwe_bake_coarse_grid     sigma_raw of the COARSE network at the cell centres, through the sigma-only path of
 *                            nwe_query_points in `precision`, in chunks, into the context's grid.  The centres are
 *                            ((float)i + 0.5f) * step + lo with step = (float)(((double)hi - (double)lo) / r): the probes = 1
 *                            arithmetic of nwe_build_occupancy and handler.grid_centres.  Synchronous: queued on `stream` and
 *                            waited for.  Refused: a host-only context, the coarse network not set (NWE_ERR_STATE); the box and
 *                            resolution as above, an unknown precision (NWE_ERR_INVALID); an MFMA precision for a shape without
 *                            a query kernel (NWE_ERR_UNSUPPORTED, the query's own message).
 *   nwe_coarse_grid_weights  test hook: the producer alone for the rays of nwe_render with these camera arguments: DEVICE
 *                            sigma_out [n_rays, n_samples] (the grid's sigma_raw per sample) and weights_out [n_rays, n_samples]
 *                            (the layout of weights_coarse); either may be NULL.  Needs a grid and nwe_set_sampling, no network.
 *                            Asynchronous on `stream`, with events of its own like nwe_create_rays. */
int nwe_set_coarse_grid(nwe_ctx *ctx, const float *lo, const float *hi, const int *res, const float *sigma, int on_device);
int nwe_clear_coarse_grid(nwe_ctx *ctx);
int nwe_get_coarse_grid(const nwe_ctx *ctx, float *lo, float *hi, int *res, float *inv);
int nwe_coarse_grid_copy(nwe_ctx *ctx, float *host_values, int64_t n_values);
int nwe_bake_coarse_grid(nwe_ctx *ctx, const float *lo, const float *hi, const int *res, int precision, void *stream);
int nwe_coarse_grid_weights(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy,
                            float near, float far, int row_begin, int row_end, float *sigma_out_dev, float *weights_out_dev,
                            void *stream);

/* Radiance grid, opt-in: a context may hold ONE radiance grid; none (the default) changes nothing.  A grid is an axis-aligned box
 * lo[3] < hi[3] in world coordinates, a resolution res = (rx, ry, rz), each axis 1..512, and rx * ry * rz rows of four fp32 values
 * (rgb_raw[3], sigma_raw) - the network's raw output, before the sigmoid and the ReLU - at the cell centres, in the layout of a
 * [rx, ry, rz, 4] array, z fastest and the four channels innermost: what handler.run_network returns at handler.grid_centres.
 * Why: a preview frame without the networks.  nwe_render_grid renders a frame by running the reference pipeline with run_network
 * replaced by a trilinear lookup in BOTH passes: no MFMA, no weight stream, a kernel bound by its gathers.  It is an entry point of
 * its own: it reads none of the modes, and nwe_render, nwe_render_rays, nwe_debug_plan and nwe_plan_report neither read the grid
 * nor refuse because of it.
 * The rule of nwe_render_grid, for each ray and each sample of EITHER pass:
 *   - the depths and points are the ones every kernel forms: coarse near * (1 - t) + far * t from the context's tables, the
 *     importance samples of sample_pdf on weights[1:-1], the merge of the two ascending lists, p = o + d * z, multiply then add,
 *     before the division by 10;
 *   - the grid coordinate, the inside test, the indices and the fraction are exactly those of the coarse grid above
 *     (nwe_set_coarse_grid, steps 2 to 4): g_c = (p_c - lo_c) * inv_c - 0.5f in three separately rounded operations, with
 *     inv_c = (float)r_c / (hi_c - lo_c) formed once on the host in fp32 (nwe_get_radiance_grid reports it); a point is outside when
 *     any p_c is not finite, or g_c < -0.5f, or g_c > r_c - 0.5f; i0 = floorf(g_c), and i0 and i0 + 1 are clamped to 0 .. r_c - 1;
 *   - INSIDE the box each of the four channels is interpolated on its own: the eight taps along z, then y, then x, each
 *     interpolation a + (b - a) * f in three separately rounded fp32 operations, no FMA (tests/radiance_grid.py restates it in
 *     numpy float32 to the same bits).  A non-finite grid value propagates in its channel;
 *   - OUTSIDE the box the row is (0, 0, 0, 0);
 *   - the row stands where run_network's row stands (nerf/models/model_utils.py:13-30): raw2outputs follows on the coarse samples,
 *     then sample_pdf, sort and raw2outputs on the n_samples + n_importance fine samples (handler.py:203-268), all of it computed
 *     with the device code the render kernels composite and sample with;
 *   - with n_importance == 0 the only pass is the output, as in nwe_render;
 *   - nwe_set_white_background is honoured.  Nothing else of the context is read: early termination, shared coarse pass, separate
 *     passes, occupancy grid, coarse grid, decomposition, work queue, colour skip, packet blocks, stamps, the one-shot hooks and
 *     the training tables are neither used nor cleared.
 * So a ray's outputs depend on the ray, the grid and the sampling tables, and on nothing else: row tiles and pose batches are
 * bit-identical to the whole call.  Flags: the rgb / depth / acc bits; the coarse bits are never raised.
 * It is an approximation.  Its size is the trilinear error of the network's raw output at the grid's resolution, plus whatever
 * the bake did to the view dependence: a grid holds one row per cell, so one direction, or a mean over directions, for all views.
 * A successful nwe_set_network / nwe_set_network_no_view_dirs of EITHER network clears the grid; a refused one leaves it.  The grid
 * calls below wait for this context's launches in flight, like nwe_set_sampling.
 *   nwe_set_radiance_grid    copies the rows (from the host or - on_device != 0 - the context's device) into a buffer the context
 *                            owns; a host-only context keeps them on the host.  Refused by name (NWE_ERR_INVALID): null pointers,
 *                            a box that is not finite or not lo < hi on every axis (or so thin that inv is not finite), a
 *                            resolution outside the domain.  If the device allocation fails (at 512^3 the grid is 2 GiB) the call
 *                            returns NWE_ERR_HIP and no grid is left set.
 *   nwe_clear_radiance_grid  no grid.
 *   nwe_get_radiance_grid    the grid's box, resolution and the fp32 inv the kernel multiplies by; any pointer may be null.
 *                            NWE_ERR_STATE (and nothing written) when no grid is set.
 *   nwe_radiance_grid_copy   the rows, n_values = 4 * rx * ry * rz, to the host.
 *   nwe_bake_radiance_grid   the raw output of network `which` at the cell centres (the probes = 1 arithmetic of nwe_build_occupancy
 *                            and handler.grid_centres), through the raw path of nwe_query_points in `precision`, in chunks through
 *                            the scratch buffer the context keeps, straight into the context's grid.  Every cell is evaluated with
 *                            the ONE direction dir3_host[3] (host memory), used as given; NULL for a network set without view
 *                            directions.  Synchronous: queued on `stream` and waited for.  Refused: a host-only context
 *                            (NWE_ERR_STATE); the box and resolution as above, `which`, an unknown precision (NWE_ERR_INVALID); the
 *                            network not set (NWE_ERR_STATE); a direction for a network without view directions or none for one
 *                            with (NWE_ERR_INVALID); an MFMA precision for a shape without a query kernel (NWE_ERR_UNSUPPORTED, the
 *                            query's own message).
 *   nwe_render_grid          the frame: the rows [row_begin, row_end) of n_poses pinhole views with the arguments of nwe_render,
 *                            into DEVICE buffers.  Needs a grid and nwe_set_sampling, and no network.  Refuses in this order,
 *                            before anything is queued: a NULL context; NULL out, a wrong struct_bytes, none of rgb / depth / acc /
 *                            the diagnostics requested (NWE_ERR_INVALID); the camera and the ray count as nwe_render refuses them;
 *                            no grid set, sampling not set (NWE_ERR_STATE); last, a host-only context (NWE_ERR_STATE) - so every
 *                            refusal in front of it can be asked of a host-only context.  Zero rays is NWE_OK and launches
 *                            nothing.  Asynchronous on `stream`; its launches have an event ring of their own, four in flight,
 *                            like the query's, which the waits of nwe_set_network / nwe_set_sampling and of the grid calls cover.
 *                            It moves none of nwe_last_kernel_ms, nwe_last_launch_parts, nwe_debug_last_plan,
 *                            nwe_last_ray_evaluations, nwe_last_coarse_launch and nwe_last_query_ms.
 *   nwe_last_grid_ms         the device time of the most recent nwe_render_grid launch that was recorded; blocks until it has
 *                            finished, like nwe_last_kernel_ms; < 0 if there was none. */
typedef struct nwe_grid_outputs {
    uint64_t struct_bytes;  /* = sizeof(nwe_grid_outputs) */
    float *rgb;             /* [R,3] */
    float *depth;           /* [R]   */
    float *acc;             /* [R]   */
    /* diagnostics, each may be NULL */
    float *weights_coarse;  /* [R, n_samples] */
    float *z_fine;          /* [R, S]      S = n_samples + n_importance: the depths of the output pass */
    float *raw_fine;        /* [R, S, 4]   the interpolated rows of the output pass */
    uint32_t *flags;        /* [1]    NWE_FLAG_RGB / _DEPTH / _ACC, OR-ed (caller zeroes it) */
} nwe_grid_outputs;
int nwe_set_radiance_grid(nwe_ctx *ctx, const float *lo, const float *hi, const int *res, const float *raw, int on_device);
int nwe_clear_radiance_grid(nwe_ctx *ctx);
int nwe_get_radiance_grid(const nwe_ctx *ctx, float *lo, float *hi, int *res, float *inv);
int nwe_radiance_grid_copy(nwe_ctx *ctx, float *host_values, int64_t n_values);
int nwe_bake_radiance_grid(nwe_ctx *ctx, const float *lo, const float *hi, const int *res, int which, const float *dir3_host,
                           int precision, void *stream);
int nwe_render_grid(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                    float far, int row_begin, int row_end, const nwe_grid_outputs *out, void *stream);
float nwe_last_grid_ms(nwe_ctx *ctx);

/* Sparse frame, opt-in: the radiance grid above as a PROPOSAL, the network only where the proposal sees weight.  An entry point of
 * its own, as nwe_render_grid is: it reads none of the modes, and no other call, plan, report or refusal knows of it.
 * The rule of nwe_render_sparse, for each ray of the call:
 *   1. Proposal.  The depths, points, grid rows, coarse weights, sample_pdf, merge and the output pass are exactly those of
 *      nwe_render_grid on the context's radiance grid and sampling tables, computed with the same device arithmetic.  S = the sample
 *      count of the output pass: n_samples + n_importance, or n_samples when n_importance == 0.  z[s], row_grid[s], w_grid[s]: its
 *      depths, its interpolated rows and the weights its compositing returns.
 *   2. Selection.  hit[s] = !(w_grid[s] <= min_weight): a NaN weight is a hit, and any min_weight < 0 hits every sample.
 *      selected[s] = the OR of hit over s - dilate .. s + dilate, clipped to 0 .. S - 1.
 *   3. Evaluation.  Every selected sample is evaluated with network `which` through the raw path of nwe_query_points in `precision`
 *      (the launcher call nwe_bake_radiance_grid makes), at the fp32 point p = o + d * z[s], multiply then add, with the ray's
 *      normalised view direction; no direction for a network set without view directions.  It does not go through nwe_query_points:
 *      nwe_last_query_ms and the query's event ring do not move.
 *   4. Output.  row[s] = the network's row where selected[s], row_grid[s] elsewhere; raw2outputs over row[.], z[.] in order, with
 *      nwe_set_white_background honoured.  Flags: the rgb / depth / acc bits only.
 * The network is not consulted outside the grid's box: a sample outside it has a zero row and a zero weight, so a ray whose samples
 * all lie outside has no hit (unless min_weight < 0) and renders as nwe_render_grid renders it.  Choose the box to hold the scene.
 * Nothing else of the context is read: no mode, hook, training table, occupancy or coarse grid.  A ray's outputs depend on the ray,
 * the grid, the sampling tables, the network and the two parameters only, so row tiles, pose batches and the chunks below are
 * bit-identical to the whole call.
 * SYNCHRONOUS: the call is queued on `stream` and waited for, as the bakes are.  The number of selected points is known only on the
 * device; it is read back once per chunk (a pinned word, a stream synchronisation) so that the query launch gets its n_points.
 * The call walks its rays in chunks of at most 2^22 / S rays (at least one), which bounds its scratch - depths, grid rows, mask,
 * compacted points, directions and query rows, about 60 bytes per sample - to about 256 MiB; the scratch is the context's own,
 * grow-only.  A chunk with no selected sample launches no query.
 * Refuses in this order, before anything is queued: a NULL context; NULL out, a wrong struct_bytes, none of rgb / depth / acc / the
 * diagnostics requested; the camera and the ray count as nwe_render refuses them; `which` not 0 or 1; an unknown precision; a NaN
 * min_weight; dilate outside 0 .. 8 (NWE_ERR_INVALID); no radiance grid; sampling not set; network `which` not set (NWE_ERR_STATE);
 * a host-only context (NWE_ERR_STATE); last, an MFMA precision for a shape without a query kernel (NWE_ERR_UNSUPPORTED, the
 * query's own message).  Zero rays is NWE_OK and launches nothing.
 * It moves none of nwe_last_kernel_ms, nwe_last_launch_parts, nwe_debug_last_plan, nwe_last_ray_evaluations,
 * nwe_last_coarse_launch, nwe_last_query_ms and nwe_last_grid_ms; its launches have an event ring of their own, which the waits of
 * nwe_set_network / nwe_set_sampling and of the grid calls cover.
 *   nwe_debug_set_sparse_chunk  test hook: the rays of a chunk; 0 = the default, otherwise at least 1 and never more than the default.
 *   nwe_last_sparse_ms          the device span of the most recent sparse call that ran (this one or nwe_render_sparse_async
 *                               below), first launch to last, the read-backs between included; < 0 if there was none.
 *   nwe_last_sparse_samples     out[0] = the samples that call selected, out[1] = its rays * S; NWE_ERR_STATE (and nothing written)
 *                               if there was none. */
typedef struct nwe_sparse_outputs {
    uint64_t struct_bytes;  /* = sizeof(nwe_sparse_outputs) */
    float *rgb;             /* [R,3] */
    float *depth;           /* [R]   */
    float *acc;             /* [R]   */
    /* diagnostics, each may be NULL */
    float *weights_coarse;  /* [R, n_samples] */
    float *z_fine;          /* [R, S]      the depths of the output pass */
    float *weights_grid;    /* [R, S]      w_grid */
    uint8_t *selected;      /* [R, S]      0 / 1 */
    float *raw_fine;        /* [R, S, 4]   the rows that were composited */
    uint32_t *flags;        /* [1]    NWE_FLAG_RGB / _DEPTH / _ACC, OR-ed (caller zeroes it) */
} nwe_sparse_outputs;
int nwe_render_sparse(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                      float far, int row_begin, int row_end, int which, int precision, float min_weight, int dilate,
                      const nwe_sparse_outputs *out, void *stream);
int nwe_debug_set_sparse_chunk(nwe_ctx *ctx, int rays);
float nwe_last_sparse_ms(nwe_ctx *ctx);
int nwe_last_sparse_samples(nwe_ctx *ctx, int64_t *out2);

/* The sparse frame, ASYNCHRONOUS, opt-in: nwe_render_sparse's arguments, rule, refusals (the same check: codes, texts and order, all
 * before anything is queued; zero rays is NWE_OK) and bits - every output and nwe_last_sparse_samples equal those of
 * nwe_render_sparse on the same context and arguments - but the call queues everything and returns, as nwe_render, nwe_render_grid
 * and nwe_query_points do.  The point count of a chunk stays on the device: the query kernels of this call read it there
 * (query_mfma_counted_kernel, query_f32_counted_kernel: a launch sized for the chunk's samples whose workgroups walk the packets
 * below the count in strides of the grid, and return at once where there is none).  A chunk with nothing selected therefore still
 * launches a query, whose workgroups all return.
 * In the steady state the call makes no read-back, no stream or event synchronisation and no blocking copy.  It waits on the host
 * only where it must: when the context's scratch has to grow, and when all four slots of the sparse ring are in flight - for the
 * sparse launches that still use them (nwe_debug_last_sparse_host_waits counts these waits).
 * One stream, one chunk buffer: the chunks, their size (2^22 / S rays; nwe_debug_set_sparse_chunk lowers it here too) and the
 * scratch are the synchronous call's, and a chunk follows the one before it in stream order.  (A second buffer with the odd chunks
 * on a side stream was measured and dropped: DESIGN.md 5.9.)  No hipGraph, no stream priorities.
 * Ordering: the call first makes `stream` wait, on the device, for the end of the previous sparse call of either kind, so two calls on
 * two streams never share the scratch.  nwe_set_network*, nwe_set_sampling, nwe_set_radiance_grid, nwe_clear_radiance_grid, the
 * bakes, nwe_render_sparse and nwe_destroy wait for it.  The outputs and the pose array (if pinned) must stay valid until `stream`
 * has passed the call.
 * Reports: nwe_last_sparse_ms and nwe_last_sparse_samples describe the most recent sparse call of either kind; after an
 * asynchronous call they wait for its end event (the tally is copied into a pinned word of the call's slot behind the last chunk).
 * No other report moves, exactly as for nwe_render_sparse.
 *   nwe_debug_last_sparse_host_waits  test hook: how many times the most recent sparse call of either kind made the host wait for
 *                                     the device: its chunks + 1 for nwe_render_sparse, 0 for a warmed asynchronous call; -1 if
 *                                     there was none.
 *   nwe_debug_query_counted_grid      the workgroups of a counted query launch (no context needed): min(ceil(capacity / packet),
 *                                     8 cus), or ceil(ceil(capacity / packet) / forced_steps) under nwe_debug_set_query_steps. */
int nwe_render_sparse_async(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                            float far, int row_begin, int row_end, int which, int precision, float min_weight, int dilate,
                            const nwe_sparse_outputs *out, void *stream);
int nwe_debug_last_sparse_host_waits(nwe_ctx *ctx);
unsigned nwe_debug_query_counted_grid(int64_t capacity, int packet, int forced_steps, int cus);

/* Adaptive frame, opt-in: render a lattice of every k-th pixel with the networks, render the pixels of the lattice cells whose
 * corners disagree as well, interpolate the rest bilinearly.  An entry point of its own, off unless called.  Every pixel that is
 * rendered has the bits nwe_render gives it; the approximation is confined to pixels whose four surrounding samples agree within
 * the caller's tolerances.  The camera arguments, R and the ray order are nwe_render's.
 * The rule, for each pose of the call on its own:
 *   Lattice.  It belongs to the rows of the CALL: lattice rows Lh = {row_begin + i k < row_end} and row_end - 1, lattice columns
 *      Lw = {i k < W} and W - 1.  A pixel with h in Lh and w in Lw is a lattice pixel (kind 0); k = 1 makes every pixel one.
 *      Consecutive lattice rows and columns bound the CELLS; with a single lattice row (or column) the cells are degenerate, h0 == h1.
 *   Stage 1.  Every lattice pixel is rendered by the networks: its ray is the row nwe_create_rays writes for it, rendered through
 *      the machinery of nwe_render_rays with rgb, depth, acc and flags requested - the bits of nwe_render for that pixel.
 *   Flat cells.  A cell is FLAT iff for every pair (i, j) of its four corner pixels fabsf(v_i - v_j) <= tol_rgb for each of r, g, b
 *      and acc, and fabsf(depth_i - depth_j) <= tol_depth: plain fp32 subtractions and comparisons, so a NaN or an inf - inf makes
 *      the cell BUSY, a tolerance below 0 makes every cell busy and +inf every cell with finite corners flat.  The rgb compared
 *      is the output rgb (behind nwe_set_white_background).
 *   Kinds.  A non-lattice pixel is RENDERED (kind 1) iff it lies in the closed rectangle [h0 .. h1] x [w0 .. w1] of at least one
 *      busy cell - a pixel on a lattice row or column between two cells is interpolated only if both are flat - and INTERPOLATED
 *      (kind 2) otherwise.
 *   Stage 2.  Every kind 1 pixel is rendered exactly as in stage 1.
 *   Stage 3.  Every kind 2 pixel is interpolated in its cell: cell row i = min(largest i with Lh[i] <= h, cells - 1), likewise the
 *      column; fy = (h1 == h0) ? 0 : (float)(h - h0) / (float)(h1 - h0), likewise fx, true fp32 divisions; each of r, g, b, depth
 *      and acc along w on the top pair and on the bottom pair, then along h, each step a + (b - a) f in three separately rounded
 *      fp32 operations (no FMA) - the arithmetic of the grids.
 *   Flags.  The rgb / depth / acc bits of both render launches, and those of any non-finite value an interpolation yields.  The
 *      coarse bits and the disparity bit are never reported.
 * So a pixel's outputs depend on the call's camera, rows, k and tolerances and on the networks only, and a pose batch is
 * bit-identical to single-pose calls.  A ROW TILE IS NOT bit-identical to the whole image near its borders: its lattice is its
 * own.  nwe_render_tiled does not use the call.
 * LIMITATION: a feature that lies wholly inside a flat cell and is narrower than k pixels is not seen (k = 2: single pixels).
 * SYNCHRONOUS: queued on `stream` and waited for, as nwe_render_sparse.  The number of kind 1 pixels is known only on the device
 * and is read back once (a pinned word) between the two render launches; a call with no busy cell makes one render launch.
 * The two render launches are ordinary render launches of the context, as two nwe_render_rays calls with lean outputs would be:
 * they take slots of the render ring, and nwe_last_kernel_ms, nwe_last_launch_parts, nwe_debug_last_plan and
 * nwe_last_ray_evaluations afterwards describe the last launch made.  Any precision; nwe_set_white_background and
 * nwe_set_separate_passes are honoured; early termination, the shared coarse pass, an occupancy grid and a baked coarse pass refuse
 * the call with nwe_render_rays' codes and texts.  The one-shot hooks and the training tables are neither used nor cleared (unlike
 * nwe_render_rays); the radiance grid is not read.
 * COST: a launch of precomputed rays is not lean, so a rendered pixel costs what a ray of nwe_render_rays costs - it pays for the
 * coarse colour and has no hollow path - not what a pixel of nwe_render costs (DESIGN.md 5.10 has the measurements).  Under
 * nwe_set_adaptive_pixel_lists (opt-in, off by default) each of the two render launches for which the list kernels of
 * nwe_render_pixels can serve the call (an MFMA precision, networks packed in a product formulation, no separate passes) hands
 * them the call's pixel list in place of a ray table: such a launch is lean, and outputs, kinds, counts and flags are the same
 * bits with the switch on and off.  Where they cannot, the call runs as without the switch.
 * The scratch (pixel lists, rays, compact outputs, kinds, counts: about 70 bytes per pixel) is the context's own, grow-only.
 * Refuses in this order, before anything is queued: a NULL context; NULL out, a wrong struct_bytes, none of rgb / depth / acc
 * requested (NWE_ERR_INVALID); the camera and the ray count as nwe_render refuses them; more than 2^24 rays; k outside 1 .. 64, a NaN
 * tolerance (NWE_ERR_INVALID); an unknown precision; everything nwe_render_rays refuses of the context for lean outputs (networks,
 * sampling, modes, shapes); last, a host-only context (NWE_ERR_STATE).  Zero rays is NWE_OK and launches nothing.
 *   nwe_last_adaptive           out4 = {pixels, lattice, rendered, interpolated} of the most recent call that ran, *ms (may be
 *                               NULL) its device span, first launch to last, the read-back gap included; NWE_ERR_STATE if none.
 *   nwe_debug_adaptive_lattice  the lattice of [first, last_excl) into out[0 .. cap): returns its size, or -1 (an empty range, k
 *                               outside 1 .. 64, NULL, cap too small).  Needs no context. */
typedef struct nwe_adaptive_outputs {
    uint64_t struct_bytes;  /* = sizeof(nwe_adaptive_outputs) */
    float *rgb;             /* [R,3] */
    float *depth;           /* [R]   */
    float *acc;             /* [R]   */
    uint8_t *kind;          /* [R]    diagnostic, may be NULL: 0 lattice, 1 rendered, 2 interpolated */
    uint32_t *flags;        /* [1]    NWE_FLAG_RGB / _DEPTH / _ACC, OR-ed (caller zeroes it) */
} nwe_adaptive_outputs;
int nwe_render_adaptive(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                        float far, int row_begin, int row_end, int precision, int k, float tol_rgb, float tol_depth,
                        const nwe_adaptive_outputs *out, void *stream);
int nwe_last_adaptive(nwe_ctx *ctx, int64_t *out4, float *ms);
int nwe_debug_adaptive_lattice(int first, int last_excl, int k, int32_t *out, int cap);
/* The switch of the COST paragraph above.  Host-side like nwe_set_separate_passes: 0 or 1, anything else is NWE_ERR_INVALID, and it
 * works on a host-only context; the getter returns -1 for a NULL context. */
int nwe_set_adaptive_pixel_lists(nwe_ctx *ctx, int on);
int nwe_get_adaptive_pixel_lists(const nwe_ctx *ctx);

/* Multi-level adaptive frame, opt-in: the adaptive frame above on a hierarchy of nested lattices - start on a coarse lattice,
 * subdivide only the cells whose corners disagree, render whole pixels only at the finest level.  An entry point of its own beside
 * nwe_render_adaptive, which it leaves as it is.  Every pixel that is rendered has the bits nwe_render gives it.  The arguments are
 * nwe_render_adaptive's, and `levels` in 1 .. 4.
 * The rule, for each pose of the call on its own:
 *   Levels.  k is the FINEST spacing.  Level l = 0 .. levels - 1 has the spacing s_l = k 2^(levels - 1 - l); s_0 must be at most 64.
 *   Lattices.  Per axis of the CALL, in local coordinates 0 .. len - 1 (rows: h - row_begin), L_l = {i s_l < len} and len - 1:
 *      nwe_render_adaptive's lattice at the spacing s_l.  The lattices are nested, L_l is a subset of L_(l+1), so every cell of
 *      level l + 1 lies inside exactly one cell of level l, its PARENT.  levels = 1 is nwe_render_adaptive's lattice.
 *   Pass 0.  Every pixel of L_0 x L_0 is rendered by the networks (kind 0).  Every level 0 cell is ACTIVE.
 *   Level l = 0 .. levels - 1.  Behind render pass l every active cell of level l is FLAT or BUSY by nwe_render_adaptive's rule on its
 *      four corners, unchanged: all pairs; r, g, b and acc within tol_rgb, depth within tol_depth; plain fp32; a NaN makes the cell
 *      busy.  Its corners are rendered by then.
 *        l < levels - 1:  the pixels of L_(l+1) x L_(l+1) that are not rendered yet and lie in the closed rectangle of at least
 *           one busy cell of level l form render pass l + 1; the children of the busy cells become active.
 *        l = levels - 1:  every pixel that is not rendered yet and lies in the closed rectangle of at least one busy cell forms
 *           render pass `levels`.
 *      The pixels of the passes 1 .. levels have kind 1.
 *   Interpolation.  Every pixel that no pass rendered has kind 2.  Its OWN cell at level l is, on both axes, cell index
 *      min(largest i with L_l[i] <= v, cells - 1) of that level's lattice.  The smallest l whose own cell is flat is taken - one
 *      exists: own cells nest, and a pixel whose own cell of the finest level is busy is rendered - and the pixel is interpolated
 *      in that cell with nwe_render_adaptive's arithmetic: fx, fy true fp32 divisions; along w on the top and on the bottom pair,
 *      then along h; each step a + (b - a) f in three separately rounded fp32 operations.
 *   Flags, modes, precisions, white background, separate passes, the hooks: as nwe_render_adaptive.
 * LIMITATION: a feature that lies wholly inside a cell that is flat at level l and is narrower than s_l pixels is not seen.  More
 * levels trade that for time: with levels = 3 and k = 2 the blind spot of a flat level 0 cell is 8 pixels wide.
 * SYNCHRONOUS, as nwe_render_adaptive.  Between two passes ONE pinned read-back of two words - the pixels of the next pass and the
 * busy cells of the level - tells the host what to launch.  A level without a busy cell ends the passes: nothing further is
 * launched, classified or read back, so a frame that is flat at level 0 costs one render launch and one read-back; a call makes at
 * the most levels + 1 render launches and `levels` read-backs.  (The interpolated counts of the report reach the host with the
 * wait that ends the call.)  A count outside its range is NWE_ERR_HIP.
 * The render launches are nwe_render_adaptive's - under nwe_set_adaptive_pixel_lists the list kernels where they can serve the
 * call, the ray table otherwise, the same bits either way; the lists are in ascending pixel order - and the render reports
 * afterwards describe the last launch made.  A ROW TILE has its own lattices: the call is not for nwe_render_tiled.
 * The scratch is the adaptive frame's own (the two calls share it, each is synchronous).
 * Refuses as nwe_render_adaptive, in its order and words, with one refusal more directly behind k: levels outside 1 .. 4, or
 * k 2^(levels - 1) > 64 (NWE_ERR_INVALID).
 *   nwe_last_adaptive_levels    out[0 .. 4 + 2 levels) = {pixels, lattice, levels, render_launches, rendered[levels] - the pixels of
 *                               the passes 1 .. levels -, interpolated[levels] - the kind 2 pixels by the level of their cell} of
 *                               the most recent call that ran, *ms (may be NULL) its device span, the read-back gaps included.
 *                               Returns NWE_ERR_INVALID where cap < 4 + 2 levels, NWE_ERR_STATE if none ran.  nwe_last_adaptive is
 *                               not moved by the call, nor this report by nwe_render_adaptive.
 *   nwe_debug_adaptive_levels_lattice   the lattice of level `level` (0 .. levels - 1) of [first, last_excl): as
 *                               nwe_debug_adaptive_lattice; -1 also for levels the call refuses.
 *   nwe_debug_adaptive_levels_plan      what a call of n_poses poses, `rows` rows and `width` columns is planned as, for a call that
 *                               is not made: out[0 .. 5 + 2 levels) = {pixels, lattice, list - the most pixels a render pass can
 *                               hold -, scratch bytes, cells[levels], pass_max[levels + 1] - the most pixels of each pass}.  Returns
 *                               the entries written, or -1 (a size below 1, more than 2^24 pixels, levels the call refuses, ray_cols
 *                               other than 8 or 11, NULL, cap too small).  Needs no context. */
typedef struct nwe_adaptive_levels_outputs {
    uint64_t struct_bytes;  /* = sizeof(nwe_adaptive_levels_outputs) */
    float *rgb;             /* [R,3] */
    float *depth;           /* [R]   */
    float *acc;             /* [R]   */
    uint8_t *kind;          /* [R]    diagnostic, may be NULL: 0 level 0 lattice, 1 rendered, 2 interpolated */
    uint32_t *flags;        /* [1]    NWE_FLAG_RGB / _DEPTH / _ACC, OR-ed (caller zeroes it) */
    uint8_t *level;         /* [R]    diagnostic, may be NULL: kind 0: 0; kind 1: its pass, 1 .. levels; kind 2: the level of its cell */
} nwe_adaptive_levels_outputs;
int nwe_render_adaptive_levels(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy,
                               float near, float far, int row_begin, int row_end, int precision, int k, int levels, float tol_rgb,
                               float tol_depth, const nwe_adaptive_levels_outputs *out, void *stream);
int nwe_last_adaptive_levels(nwe_ctx *ctx, int64_t *out, int cap, float *ms);
int nwe_debug_adaptive_levels_lattice(int first, int last_excl, int k, int levels, int level, int32_t *out, int cap);
int nwe_debug_adaptive_levels_plan(int n_poses, int rows, int width, int k, int levels, int ray_cols, int64_t *out, int cap);

/* Pixel list: render any subset of the pixels of a pinhole view, in any order, on lean kernels.
 * The camera arguments are nwe_render's.  pixels_dev[i] is an output ray index of nwe_render with the same camera arguments,
 * (p * (row_end - row_begin) + (h - row_begin)) * W + w, and output row i holds, bit for bit, what nwe_render writes to that row.
 * Any order; duplicates are allowed.  A value outside [0, n_poses * rows * W) renders the clamped pixel (below 0: pixel 0, else the
 * last): defined, and never an out-of-range read.
 * Flags.  Only the rgb / depth / acc bits are reported, whichever path ran (the adaptive frame's rule): the launch raises its bits
 * into a word of its slot's and a one-thread kernel ORs the masked word into the caller's.
 * ASYNCHRONOUS on `stream`, like nwe_render: poses are staged before the call returns; the list must stay valid until the stream
 * has passed the call.  The call is an ordinary launch on the render ring: nwe_last_kernel_ms, nwe_last_launch_parts,
 * nwe_debug_last_plan and nwe_last_ray_evaluations (executed == full) describe it.  nwe_set_white_background is honoured.
 * PATH.  Under an MFMA precision, when the one shape both networks share has list kernels - both are packed in a product
 * formulation - and separate passes are off, the call takes the LIST KERNELS: the lean kernels of nwe_render (density-only coarse
 * pass, hollow colour path, both work decompositions, the work queue) that read each ray's pixel from the list.  The launch is
 * planned as the same number of rays of nwe_render_rays is: no packet blocks, no tail path.  Every other legal call - NWE_PREC_F32,
 * separate passes, a network packed unfolded (nwe_debug_set_fold(0)), a shape without list kernels - renders through a RAY TABLE:
 * the rows nwe_create_rays writes for the clamped pixels, into a buffer the launch's slot owns, then nwe_render_rays' launch.  The
 * bits are the same; the cost is that of nwe_render_rays.  nwe_last_pixels says which path the last launch took (path: 1 list
 * kernels, 0 ray table; a render launch of nwe_render_adaptive under nwe_set_adaptive_pixel_lists counts as one); NWE_ERR_STATE if
 * none ran.  nwe_debug_pixels_path answers for a call that is not made: 1 / 0, -1 for a NULL context or an unknown precision; a
 * host-only context serves it.
 * Refuses in this order, before anything is queued: a NULL context; NULL out, a wrong struct_bytes, none of rgb / depth / acc
 * requested (NWE_ERR_INVALID); the camera and its ray count as nwe_render refuses them; n_pixels < 0 or >= 2^31, or NULL pixels_dev
 * with n_pixels > 0 (NWE_ERR_INVALID); an unknown precision; everything nwe_render_rays refuses of the context for lean outputs, in
 * its codes and texts (networks, sampling, shapes; early termination, the shared coarse pass, an occupancy grid and a baked coarse
 * pass); last, a host-only context (NWE_ERR_STATE).  n_pixels == 0 is NWE_OK and launches nothing.  The one-shot hooks and the
 * training tables are neither used nor cleared. */
typedef struct nwe_pixel_outputs {
    uint64_t struct_bytes;  /* = sizeof(nwe_pixel_outputs) */
    float *rgb;             /* [n,3] */
    float *depth;           /* [n]   */
    float *acc;             /* [n]   */
    uint32_t *flags;        /* [1]    NWE_FLAG_RGB / _DEPTH / _ACC, OR-ed (caller zeroes it) */
} nwe_pixel_outputs;
int nwe_render_pixels(nwe_ctx *ctx, const float *c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                      float far, int row_begin, int row_end, const int32_t *pixels_dev, int64_t n_pixels, int precision,
                      const nwe_pixel_outputs *out, void *stream);
int nwe_last_pixels(nwe_ctx *ctx, int64_t *n_pixels, int *path);
int nwe_debug_pixels_path(const nwe_ctx *ctx, int precision);

/* The producer launch of the most recent render launch (the one nwe_last_kernel_ms describes, under the same rules; blocks like
 * it): *ms = its time, *rays = the representative rays it walked; -1 / 0 when that launch had none (k = 1 without separate
 * passes, n_importance == 0, or a call armed with nwe_debug_set_coarse_weights).  Under separate passes with k = 1 it is the
 * coarse launch and *rays the call's rays; under a baked coarse pass (nwe_set_coarse_grid) the grid producer and the call's rays.
 * nwe_last_kernel_ms spans both launches, nwe_last_launch_parts describes the consumer's. */
int nwe_last_coarse_launch(nwe_ctx *ctx, float *ms, int64_t *rays);

/* Ray evaluations of the most recent render launch of this context (the launch nwe_last_kernel_ms describes, under the same
 * rules about refused calls; blocks like it): out[0] = executed, counted as the rays of each workgroup times the samples
 * that workgroup walked, out[1] = the full count n_rays * (n_samples [+ n_samples + n_importance]).  A launch without early
 * termination reports out[0] == out[1], except under a shared coarse pass (nwe_set_shared_coarse, k > 1 and n_importance > 0),
 * where out[0] = n_rep * n_samples + n_rays * (n_samples + n_importance) for the n_rep representatives of the call, and under an
 * occupancy grid (nwe_set_occupancy), which counts the iterations each group of rays evaluated.  Shows the skip without a clock. */
int nwe_last_ray_evaluations(nwe_ctx *ctx, int64_t *out2);

/* Training-mode forward (nerf/training/nerf_replica_training_handler.py:553-580; forward only): the NEXT
 * nwe_render_rays call uses random numbers drawn by the caller exactly where the reference calls torch.rand /
 * torch.randn, one row per ray of that call (DEVICE pointers, each may be NULL = the inference behaviour); cleared
 * after that call.
 *   t_rand       [n_rays, n_samples]                stratified jitter in [0,1): z = lower + (upper - lower) * t_rand (:553-562)
 *   noise_coarse [n_rays, n_samples]                added to sigma_raw before the ReLU, i.e. randn * raw_noise_std
 *   noise_fine   [n_rays, n_samples + n_importance] (nerf/models/model_utils.py:64-71)
 *   u_sorted     [n_rays, n_importance]             the uniform numbers of sample_pdf(det=False) (nerf/rays/rays.py:98),
 *                                                   sorted ascending per ray: sample_pdf is element-wise in u and the
 *                                                   reference sorts the union of depths afterwards (:580), so the order of
 *                                                   u does not change any output
 * A table row belongs to its ray: row i of every table is read for ray i of the call, whatever packet, workgroup, work item or
 * launch of the call's plan the ray lands in, so a call over rays [a, b) of a larger call with rows [a, b) of its tables gives
 * rows [a, b) of the larger call's outputs bit for bit.  A noise table of 0.0 and a u_sorted equal to the u of nwe_set_sampling
 * give the inference result bit for bit.  With n_importance == 0, noise_fine and u_sorted are not read.
 * Tables together with the one-shot hooks above - a hook replaces its stage and nothing else, in both kernels:
 *   nwe_debug_set_coarse_weights  the coarse pass does not run, so noise_coarse has nothing to act on (the call equals the call
 *                                 without it bit for bit); t_rand still defines the coarse depths and with them the bin edges
 *                                 z_mid and the coarse members of z_fine; u_sorted is used as ever;
 *   nwe_debug_set_raw             noise_coarse / noise_fine are added to the CALLER's sigma_raw of that pass before the ReLU;
 *                                 t_rand and u_sorted are used as ever (the depths enter the compositing and z_fine);
 *   nwe_debug_set_fine_depths     the fine pass runs at the caller's depths with noise_fine; the importance samples feed nothing
 *                                 into it, so rgb / depth / acc / raw_fine / z_fine do not depend on u_sorted, but z_std and
 *                                 sample_cond / sample_amp / sample_switch still describe the call's OWN importance samples
 *                                 (drawn with u_sorted, from the call's coarse weights), not the caller's depths.
 * (tests/train_domain.py lists the cases.) */
int nwe_set_train_tables(nwe_ctx *ctx, const float *t_rand_dev, const float *noise_coarse_dev, const float *noise_fine_dev,
                         const float *u_sorted_dev);

/* Test hook: the MFMA kernel has two work decompositions with bit-identical results (four ray packets per workgroup, or
 * one packet whose samples are dealt to the four waves) and picks by frame size - all of one kind, or the full rounds of
 * workgroups as packets and the ragged last round sample-split in a second launch; mode 0 / 1 / 2 forces a plan, -1
 * restores the automatic choice. */
int nwe_debug_set_decomposition(nwe_ctx *ctx, int mode);
/* The plan the most recent MFMA launch of this context took (0 packets / 1 sample split / 2 packets + split rest), -1 if
 * none yet: lets a test check the launcher's choice without timing anything. */
int nwe_debug_last_plan(const nwe_ctx *ctx);

/* How the workgroups of a plain MFMA launch get their work ("Dealing"; bit-identical results).  The hardware
 * hands workgroup b of a launch to XCD (b + c) mod 8: an eighth of the launch per XCD, whatever pace the XCD runs at, and the
 * launch ends with the slowest.  A QUEUED launch of n work items instead starts nwe_debug_queue_grid(n) workgroups, each of
 * which takes a ticket from a counter as its first act and renders that item - or leaves at once if the ticket is not below
 * n - so a faster XCD takes more of the frame.  Under the hybrid plan with queues on, the sample-split launch is also sent to
 * a low-priority stream of the context's own that forks from the caller's stream in front of the packets launch and is
 * joined behind it: its quarter-size items fill the CUs that have run out of packets while the slowest XCD finishes.
 *   mode -1 (default): queue a launch that has more workgroups than the device has CUs
 *   mode  0: never queue - the hardware's dealing, grid for grid
 *   mode  1: queue every plain MFMA launch whatever its size (tests)
 * NWE_WORK_QUEUE=0 / 1 in the environment sets the mode a new context starts with; NWE_WORK_QUEUE_BACKFILL=0 keeps a new
 * context's second launch on the caller's stream behind the first (A/B timing of the backfill on one library).  Early termination, the shared coarse pass,
 * separate passes and NWE_PREC_F32 keep their launches as they are and report no queue.
 * nwe_last_launch_parts under a backfilled hybrid plan: ms2[0] is the packets launch as before; ms2[1] is how long the frame
 * ran BEYOND its first launch, not the time of the second launch (which ran beside the first), so a rate computed from it
 * means nothing.  Both stay positive and add up to nwe_last_kernel_ms to within the timer's step: the three events lie on the
 * caller's stream in order, the last behind the join, and a part below that step is reported as the step (1e-5 ms).
 * The tail path: a lean call under the hybrid plan whose packets launch is queued, with the backfill on, and whose surplus
 * workgroups - nwe_debug_queue_grid(items) - items of the packets launch - are at least as many as the sample-split items, renders
 * those items in the packets launch itself: a surplus workgroup, instead of leaving at once, takes a number from a third counter
 * and renders that split item.  The surplus is placed when the packet tickets have run out, so the split items sit at the
 * end of the frame, on the CUs that come free first.  The second launch stays - same grid, counter and stream, now forked
 * behind the first launch - and renders the items whose number is not below the third counter's final value: none.  Nothing
 * waits for anything.  items, grid, taken and side_stream of nwe_debug_last_queue are what they are without the path.
 * nwe_last_launch_parts then: ms2[0] is the packets launch INCLUDING the split items, ms2[1] the few microseconds of the emptied
 * second launch; rays2 is unchanged.  NWE_WORK_QUEUE_TAIL=0 in the environment keeps a new context off the path (A/B timing).  There
 * is NO run-time switch: the variable is read once, by nwe_create, and holds for the context's life (nwe_debug_get_work_queue_tail);
 * NWE_WORK_QUEUE_BACKFILL=0 does so too.  Every other call - not lean, a smaller surplus, early termination, shared coarse pass,
 * separate passes - runs the launches it ran without the path. */
int nwe_debug_set_work_queue(nwe_ctx *ctx, int mode);
int nwe_debug_get_work_queue(const nwe_ctx *ctx);               /* -2 for a null context */
int nwe_debug_get_work_queue_backfill(const nwe_ctx *ctx);      /* 1, or 0 under NWE_WORK_QUEUE_BACKFILL=0; -1 for a null context */
/* The grid of a queued launch of `items` work items: items plus a quarter, rounded up to a multiple of 8.  No device needed. */
unsigned nwe_debug_queue_grid(unsigned items);
/* The plan of a render call without the call: what nwe_render (n_rays < 0: the camera's n_poses, H, W and rows
 * [row_begin, row_end)) or nwe_render_rays (n_rays >= 0; the camera arguments are not read) would decide for this context
 * on a device of `cus` compute units.  The context may be host-only; its state is read as it is: networks, sampling, early
 * termination, shared coarse pass, separate passes, decomposition, work-queue mode, backfill and tail.  Of `out` only null /
 * non-null is read; `hooks` says which one-shot hooks of nwe_render_rays count as armed (the context's own stay as they are).
 * Returns the refusal the real call would return for these arguments, with its text (nwe_last_error), a host-only context's
 * own refusal aside; else fills *report, whose struct_bytes the caller has set.  Touches no device, launches nothing, moves
 * no ring.  A call of no rays plans nothing: the report is zero. */
#define NWE_PLAN_HOOK_COARSE_WEIGHTS 1u /* nwe_debug_set_coarse_weights */
#define NWE_PLAN_HOOK_OTHER 2u          /* any of nwe_debug_set_fine_depths / _raw, nwe_set_train_tables */
/* One stage of the call - the coarse launch of a shared coarse pass or of separate passes, or the main stage every call has -
 * and, for the MFMA precisions, the plan of its launches. */
typedef struct nwe_plan_stage {
    int32_t active;       /* 0: the call has no such stage, and the rest is zero */
    int32_t role;         /* 0 one fused kernel, 1 producer (coarse pass alone), 2 consumer (fine pass alone) */
    int64_t n_rays;       /* the stage's rays: the producer's are the representatives */
    int32_t n_importance;
    int32_t net;          /* the network (0 coarse, 1 fine) in both descriptor slots, -1: (coarse, fine) */
    int32_t variant;      /* the kernels: 0 plain, 1 terminating, 2 sharing, 3 occupancy grid, 5 pixel list (nwe_render_pixels); -1: the grid producer of a baked coarse pass */
    int32_t plan;         /* nwe_debug_last_plan: 0 packets, 1 sample split, 2 packets + split rest; -1: that producer, which has none */
    int32_t n_launches;   /* 1, or 2 under plan 2 */
    int32_t fork;         /* 0 the second launch follows the first on the caller's stream; it goes to the side stream, which forks
                             1 in front of the first launch (backfill), 2 behind it (tail path) */
    int64_t ray_first[2], rays[2];   /* per launch: its rays, */
    int32_t split[2];                /* 1 = one packet per work item, 0 = four, */
    uint32_t items[2], grid[2];      /* its work items, and its grid if it is queued (0: dealt by the hardware) */
    int32_t tail;         /* 1: the tail path is taken */
    uint32_t tail_items;  /* ... and the split items it renders in the packets launch */
} nwe_plan_stage;
typedef struct nwe_plan_report {
    uint64_t struct_bytes;
    int32_t separate, share, full;      /* two launches with each network's own kernels; through the sharing kernels; the full ones */
    int32_t coarse_launch;              /* the call has a coarse stage */
    int32_t may_queue, need_side;       /* a launch is queued: the slot's counters are zeroed; the side streams exist */
    int32_t need_evals, coarse_flags;   /* the slot's evaluation counter is zeroed; the coarse launch has a flag word of its own */
    int32_t share_k, reserved;
    int64_t table_elems;                /* floats of the slot's weight table between the two stages */
    int64_t evals_full, evals_run;      /* nwe_last_ray_evaluations [1] and, without early termination, [0] */
    int64_t share_rays;                 /* nwe_last_coarse_launch */
    nwe_plan_stage coarse, main;
} nwe_plan_report;
int nwe_debug_plan(nwe_ctx *ctx, int n_poses, int H, int W, int row_begin, int row_end, int64_t n_rays, const nwe_outputs *out,
                   unsigned hooks, int precision, int cus, nwe_plan_report *report);
/* The most recent recorded render launch of this context, per launch of its plan: its work items, its grid and the final value
 * of its ticket counter (= grid when every workgroup took one); zeros = not queued.  *side_stream (may be NULL): 1 if the
 * second launch ran on the context's low-priority stream.  Waits for the launch, like the timing calls. */
int nwe_debug_last_queue(nwe_ctx *ctx, unsigned *items2, unsigned *grid2, unsigned *taken2, int *side_stream);
int nwe_debug_get_work_queue_tail(const nwe_ctx *ctx);          /* 1, or 0 under NWE_WORK_QUEUE_TAIL=0; -1 for a null context */
/* *stolen: the sample-split items that the packets launch of the most recent recorded render launch rendered in its tail (all
 * of them when the tail path was taken), 0 when it was not.  Waits for the launch, like the timing calls. */
int nwe_debug_last_tail(nwe_ctx *ctx, unsigned *stolen);
/* *rendered: the sample-split items that the SECOND launch of that render launch rendered on the tail path (the ones whose number
 * was not below the third counter's final value), 0 when the path was not taken.  stolen + rendered == the plan's split items
 * says that every item was rendered exactly once; with the path's condition (the surplus covers every item) rendered is 0. */
int nwe_debug_last_tail_rest(nwe_ctx *ctx, unsigned *rendered);

/* The hollow path of the lean MFMA kernels ("Samples without density"): in the pass that produces the
 * outputs, a wave whose 32 rays all have sigma_raw <= 0 at a sample leaves out the colour layers of that evaluation - the
 * sample weighs 0 on every one of them.  No bit of any output changes wherever the colour the full path computes there is not
 * NaN; the one deliberate difference is named in DESIGN.md.
 *   mode 0: off - every evaluation runs the colour layers
 *   mode 1 (default): on for a network whose colour layers are finite as packed (nwe_packed_colour_finite) and for waves whose
 *           rays all have finite view directions
 *   mode 2: test hook - as 1 without the pack-time condition, so that a NaN planted in the colour head shows where the path ran
 * NWE_COLOUR_SKIP=0 / 1 in the environment sets the mode a new context starts with.  Calls that are not lean, NWE_PREC_F32, the
 * unfolded and the no-view-dirs formulations and nwe_query_points have no such path. */
int nwe_debug_set_colour_skip(nwe_ctx *ctx, int mode);
int nwe_debug_get_colour_skip(const nwe_ctx *ctx);              /* -1 for a null context */

/* Packets of 8x4 pixel blocks ("Samples without density"): in a lean nwe_render call on the plain MFMA
 * kernels (no early termination, shared or baked coarse pass, occupancy grid or separate passes) whose rows per pose are a
 * multiple of 4 and whose W is a multiple of 8, the 32 rays of a wave are one block of 8 columns x 4 rows instead of 32
 * consecutive pixels of a row, so that the hollow path above is taken more often.  No bit of any output depends on it.
 * on = 1 (default) / 0; NWE_PACKET_BLOCKS=0 / 1 in the environment sets what a new context starts with.
 * nwe_debug_last_packet_blocks: 1 / 0 = the call most recently planned on this context - rendered, or asked about with
 * nwe_debug_plan - was / was not blocked; -1 for a null context.
 * nwe_debug_packet_pixels: pixels[i] = the pixel index (row-major over [pose][row][column] of the call) that ray index first + i
 * of a blocked call of width W names; needs no context. */
int nwe_debug_set_packet_blocks(nwe_ctx *ctx, int on);
int nwe_debug_last_packet_blocks(const nwe_ctx *ctx);
int nwe_debug_packet_pixels(int64_t first, int64_t n, int W, int32_t *pixels);

/* Diagnostic builds only (make -C csrc stamps): DEVICE buffer of 14 uint64 per wave that a -DNWE_STAMPS build of the MFMA
 * kernel fills with s_memtime cycle sums (tools/stamp_run.py); the product build never touches it.  NULL switches it off.
 * Row = (work item of its launch) * 4 + wave, however the items were dealt (nwe_debug_set_work_queue), and the rows of the hybrid
 * plan's second launch follow the first's: the buffer holds 4 rows per work item of the call, i.e. 4 * ceil(rays / 128) for a
 * packets launch plus 4 * ceil(rays / 32) for a sample-split one, whatever the grid.  Words 0-7:
 * cycle sums per segment, 8: the wave's lifetime in 100 MHz ticks (s_memrealtime), 9: s_memtime at its start, 10:
 * HW_REG_XCC_ID (the XCD: low four bits) | HW_REG_HW_ID << 32, 11: the work item it rendered, 12 / 13: its start / end on
 * the 100 MHz clock. */
int nwe_debug_set_stamps(nwe_ctx *ctx, unsigned long long *per_wave_dev);

/* Device self-test of the hardware assumptions the MFMA kernel relies on (fragment layouts of
 * v_mfma_f32_32x32x16_f16, fp16 subnormal operands, LDS-DMA lane order).  report[0..7] receives
 * mismatch counts / measured values (report[4] / report[7]: the positional encoding's error against fp64 over scene-sized
 * arguments / over its whole documented range, in 1e-9; report[7] = -1 if an argument beyond the range gave a finite value);
 * returns NWE_OK when every assumption holds. */
int nwe_selftest(nwe_ctx *ctx, int32_t *report8);

#ifdef __cplusplus
}
#endif
#endif /* NWE_H */
