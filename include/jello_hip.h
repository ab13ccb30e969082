/* jello_hip.h -- C ABI of libjello_hip.so, the MI355X (gfx950) replacement for Jello's
 * engine/wgpu_engine.  These are exactly the entry points a Go `engine/hip_engine` package binds
 * with cgo to replay a renderer.Recording (see INTEGRATION.md for the cgo stub).
 *
 * Mapping to the reference interface each call replaces:
 *   jh_create / jh_destroy        wgpu_engine.New                      engine/wgpu_engine/wgpu.go:157-178
 *   jh_upload                     Upload / UploadUniform commands      wgpu.go:353-370 (queue.WriteBuffer)
 *   jh_image_upload               UploadImage command                  wgpu.go:372-418
 *   jh_clear                      Clear command                        wgpu.go:565-585
 *   jh_dispatch                   Dispatch command                     wgpu.go:454-497
 *   jh_dispatch_indirect          DispatchIndirect command             wgpu.go:499-552
 *   jh_download                   Download command + map               wgpu.go:554-563, 645-657
 *   jh_free / jh_image_free       FreeBuffer / FreeImage (pool return) wgpu.go:587-616, 772-808
 *   jh_image_import/buffer_import ExternalResource{ExternalImage,..}   wgpu.go:81-93, lib.go:257-262
 *   jh_image_write                WriteImage command                   wgpu.go:422-452 (queue.WriteTexture)
 *   jh_profile_enable/collect     ProfilerGroup.Compute timestamps     engine/wgpu_engine/profiler.go:160-177
 *   jh_profile_group_begin/end    Profiler.Start / Nest / End          profiler.go:49-65, 113-158
 *   jh_profile_collect_tree       Profiler.Collect (nested results)    profiler.go:304-385
 *   jh_stage                      renderer.FullShaders field order     renderer/render.go:17-43
 *   jh_blit                       RenderToSurface's blit pass          engine/wgpu_engine/lib.go:109-198, 266-333
 *   jh_blit_yuv                   (no counterpart: the same target as NV12 / I420 video frames)
 *   jh_pack_tiles / jh_unpack_tiles   (no counterpart: the frame's way off the GPU)
 *   jh_dash                           (no counterpart: the reference dashes on the CPU with curve.Dash)
 *   jh_blur                           (no counterpart: Gaussian blur of the RGBA16F target on the device)
 *   jh_resample                       (no counterpart: an RGBA16F image resized on the device, four filters)
 *   jh_composite                      (no counterpart: one RGBA16F image blended onto another on the device)
 *   jh_color_filter                   (no counterpart: colour matrix and transfer functions on an RGBA16F image)
 *   jh_morphology                     (no counterpart: erode / dilate of an RGBA16F image by a box on the device)
 *   jh_warp                           (no counterpart: an affine transform of an RGBA16F image on the device)
 *   jh_convolve                       (no counterpart: feConvolveMatrix on an RGBA16F image on the device)
 *   jh_lighting                       (no counterpart: feDiffuseLighting / feSpecularLighting on the device)
 *   jh_turbulence                     (no counterpart: feTurbulence noise into an RGBA16F image on the device)
 *   jh_displace                       (no counterpart: feDisplacementMap on RGBA16F images on the device)
 *   jh_shadow                         (no counterpart: a blurred rounded rectangle generated into an RGBA16F image)
 *   jh_perspective                    (no counterpart: a projective transform of RGBA16F images on the device)
 *   jh_distance                       (no counterpart: the capped Euclidean distance to a shape, through a ramp)
 *   jh_stats                          (no counterpart: content bounds, channel extremes and histograms of an RGBA16F image)
 *   jh_lut3d                          (no counterpart: a 3D colour lookup table applied to an RGBA16F image on the device)
 * Binding order for every stage is the WGSL @binding order = renderer/render.go dispatch order.
 *
 * Conventions: plain pointers and sizes only; every call returns 0 on success or a negative
 * jh_status (never aborts -- the reference panics, wgpu.go:77,213,282,544,558,594,955);
 * one jh_ctx = one device + one stream, not thread-safe; several contexts (one per GPU -- or two on
 * ONE GPU that take a stream of frames in turn, which fills the holes a single chain of dependent
 * launches leaves: INTEGRATION.md) may be used concurrently.  Work is enqueued asynchronously; only
 * jh_download, jh_image_download, jh_sync and jh_profile_collect[_tree] wait for the device.
 * Uploads copy the caller's bytes into a pinned staging arena before returning (the slice may be
 * reused at once, as with queue.WriteBuffer) and leave the DMA in flight.
 */
#ifndef JELLO_HIP_H
#define JELLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jh_ctx jh_ctx;

typedef enum jh_status {
    JH_OK = 0,
    JH_ERR_INVALID = -1,     /* bad argument / unknown id / wrong binding count */
    JH_ERR_DEVICE = -2,      /* HIP runtime error (jh_last_error has the text) */
    JH_ERR_NO_DEVICE = -3,   /* no usable GPU */
    JH_ERR_UNSUPPORTED = -4, /* stage not implemented by this build */
    JH_ERR_OOM = -5
} jh_status;

/* renderer.FullShaders field order (renderer/render.go:17-43) */
typedef enum jh_stage {
    JH_PATHTAG_REDUCE = 0,
    JH_PATHTAG_REDUCE2 = 1,
    JH_PATHTAG_SCAN1 = 2,
    JH_PATHTAG_SCAN_SMALL = 3,
    JH_PATHTAG_SCAN_LARGE = 4,
    JH_BBOX_CLEAR = 5,
    JH_FLATTEN = 6,
    JH_DRAW_REDUCE = 7,
    JH_DRAW_LEAF = 8,
    JH_CLIP_REDUCE = 9,
    JH_CLIP_LEAF = 10,
    JH_BINNING = 11,
    JH_TILE_ALLOC = 12,
    JH_BACKDROP_DYN = 13,
    JH_PATH_COUNT_SETUP = 14,
    JH_PATH_COUNT = 15,
    JH_COARSE = 16,
    JH_PATH_TILING_SETUP = 17,
    JH_PATH_TILING = 18,
    JH_FINE_AREA = 19,
    JH_FINE_MSAA8 = 20,
    JH_FINE_MSAA16 = 21,
    JH_STAGE_COUNT = 22
} jh_stage;

/* renderer.ResourceProxy (renderer/recording.go:23-36) */
typedef enum jh_binding_kind { JH_BIND_BUFFER = 1, JH_BIND_IMAGE = 2, JH_BIND_IMAGE_ARRAY = 3 } jh_binding_kind;
typedef struct jh_binding {
    uint32_t kind;       /* jh_binding_kind */
    uint32_t count;      /* JH_BIND_IMAGE_ARRAY: number of ids */
    uint64_t id;         /* buffer / image ResourceID */
    const uint64_t* ids; /* JH_BIND_IMAGE_ARRAY */
} jh_binding;

typedef struct jh_profile_record {
    int32_t stage; /* jh_stage */
    uint32_t pad;
    float ms; /* device time of the whole stage (all of its kernels), hipEvent pair */
} jh_profile_record;

/* One node of the nested profile (ProfilerResult, profiler.go:289-302): a group (label, CPU interval, children) or a GPU
 * query (one per dispatch, label = the stage's name as in wgpu.go:486).  Nodes come in creation order, so a node's
 * parent always precedes it; times are milliseconds relative to the first node (CPU clock) / the first query (GPU). */
typedef enum jh_profile_kind { JH_PROF_GROUP = 0, JH_PROF_QUERY = 1 } jh_profile_kind;
typedef struct jh_profile_node {
    int32_t kind;   /* jh_profile_kind */
    int32_t parent; /* index of the enclosing group in the same array, -1 at top level */
    int32_t stage;  /* query: jh_stage; group: -1 */
    uint32_t pad;
    char label[48];
    double cpu_start_ms, cpu_end_ms; /* group: Start/Nest .. End; query: the enqueue call */
    float gpu_start_ms, gpu_end_ms;  /* query: its hipEvent pair; group: hull of the queries below it (0,0 if none) */
} jh_profile_node;

/* ---- context ---- */
int jh_create(jh_ctx** out, int device);
void jh_destroy(jh_ctx* ctx);
const char* jh_last_error(jh_ctx* ctx);
const char* jh_stage_name(int stage);
/* Run on a caller-owned HIP stream (e.g. torch's current stream); NULL = the context's own. */
int jh_set_stream(jh_ctx* ctx, void* hip_stream);
/* A stream of the lowest (level < 0), default (0) or highest (> 0) launch priority of the context's device -- for a caller that puts
 * a stage on a stream of its own (no reference counterpart; tools/fine_priority.py).  jh_stream_destroy releases it. */
int jh_stream_create(jh_ctx* ctx, int level, void** hip_stream);
int jh_stream_destroy(jh_ctx* ctx, void* hip_stream);
int jh_sync(jh_ctx* ctx);
/* Band mode (sharding ONE target over several GPUs): this context writes the PTCL and rasterises only the
 * bin rows [bin_row0, bin_row1) (a bin row = 16 tile rows = 256 pixel rows).  Every other stage, and the counting pass
 * of coarse, still covers the whole scene, so all allocation offsets -- hence every PTCL word and segment index of the
 * band -- are those of the unsharded run; the target image is written in the band's rows only.  (0, UINT32_MAX) = whole
 * target (default).  The reference has no counterpart: one wgpu device renders the whole target (render.go:399-434). */
int jh_set_band(jh_ctx* ctx, uint32_t bin_row0, uint32_t bin_row1);
/* Optional: an upper bound of the nesting depth of clip / blend layers (open BEGIN_CLIPs at any point of the draw tag stream)
 * in the recordings run next; 0 = unknown.  fine keeps the blend-stack levels between its own LDS level and the WGSL's
 * blend_spill (fine.wgsl:938-949, BLEND_STACK_SPLIT = 4) in a per-tile scratch slice of 4 KiB per level: without the hint it
 * reserves the worst case, three levels (768 MiB for a 4096 x 4096 target), with it 0 / 1 / 2 / 3 levels for depth <= 1 / 2 /
 * 3 / >= 4.  A hint that is too SMALL loses the saved colours of the deeper levels (wrong pixels, no out-of-bounds access).  The
 * engine shims count the depth off encoding.DrawTags in RenderToTexture; the reference has no counterpart (its blend stack is
 * `var blend_stack: array<array<vec4<f32>, 4>, 4>` in registers). */
int jh_set_clip_depth_hint(jh_ctx* ctx, uint32_t max_depth);
/* Blend-stack saves fine dropped since the last reset because the hint above was smaller than the scene's real nesting depth
 * (each one is a wrong pixel colour; memory safety is never at stake): 0 after every frame rendered with a correct hint or
 * with no hint.  A caller that sets hints should check it in debug builds.  Synchronises the context's stream. */
int jh_debug_clip_hint_overflows(jh_ctx* ctx, uint32_t* count, int reset);

/* ---- buffers (ids are the recording's ResourceIDs; sizes in bytes) ---- */
int jh_buffer_create(jh_ctx* ctx, uint64_t id, uint64_t size);
int jh_buffer_import(jh_ctx* ctx, uint64_t id, void* device_ptr, uint64_t size); /* caller keeps ownership */
int jh_upload(jh_ctx* ctx, uint64_t id, const void* data, uint64_t size);        /* creates the buffer if needed */
int jh_clear(jh_ctx* ctx, uint64_t id, uint64_t offset, int64_t size);           /* size < 0: to the end */
int jh_download(jh_ctx* ctx, uint64_t id, void* dst, uint64_t offset, uint64_t size);
int jh_free(jh_ctx* ctx, uint64_t id); /* returns the allocation to the pool */
void* jh_buffer_device_ptr(jh_ctx* ctx, uint64_t id);
uint64_t jh_buffer_size(jh_ctx* ctx, uint64_t id);

/* ---- images: linear device memory, row-major, format = renderer.ImageFormat ----
 * An image that was only created (never uploaded / imported), or whose upload was all zero bytes (the 1x1 placeholder
 * of render.go:115-124), samples as transparent black like a fresh wgpu texture.  JL_RGBA8_SRGB texels are decoded to
 * linear when fine samples them (an rgba8unorm-srgb texture view); alpha is linear. */
int jh_image_create(jh_ctx* ctx, uint64_t id, uint32_t width, uint32_t height, int format);
int jh_image_import(jh_ctx* ctx, uint64_t id, void* device_ptr, uint32_t width, uint32_t height, int format);
int jh_image_upload(jh_ctx* ctx, uint64_t id, uint32_t width, uint32_t height, int format, const void* data, uint64_t size);
/* WriteImage: `data` holds height rows of width texels, tightly packed; written to the rectangle at (x, y). */
int jh_image_write(jh_ctx* ctx, uint64_t id, uint32_t x, uint32_t y, uint32_t width, uint32_t height, const void* data, uint64_t size);
int jh_image_download(jh_ctx* ctx, uint64_t id, void* dst, uint64_t size);
int jh_image_free(jh_ctx* ctx, uint64_t id);
void* jh_image_device_ptr(jh_ctx* ctx, uint64_t id);
/* The size an image was created, uploaded or imported with (either pointer may be null); JH_ERR_INVALID for an unknown id, with no message. */
int jh_image_size(jh_ctx* ctx, uint64_t id, uint32_t* width, uint32_t* height);

/* ---- dispatch ----
 * One call per recorded Dispatch: `stage` is a jh_stage (= the field order of renderer.FullShaders), (gx, gy, gz) the
 * recorded workgroup counts, bindings in WGSL @binding order.  All 22 stages are implemented (fine_msaa8/16 included).
 * Several stages pick a specialised instantiation from the HOST SHADOW of the ConfigUniform that was uploaded to the
 * buffer bound at index 0 (n_clip == 0: no clip stack) and from what is bound (no ramp / no non-zero image: no
 * gradient code); a config that only exists on the device selects the general instantiation. */
int jh_dispatch(jh_ctx* ctx, int stage, uint32_t gx, uint32_t gy, uint32_t gz, const jh_binding* bindings, int n_bindings);
int jh_dispatch_indirect(jh_ctx* ctx, int stage, uint64_t indirect_buffer_id, uint64_t offset, const jh_binding* bindings,
                         int n_bindings);

/* ---- hipGraph capture of a replayed recording (a frame is ~35 short launches: launch-bound on the host) ----
 * jh_graph_begin starts capturing everything enqueued on the context's stream (dispatches, clears);
 * jh_graph_end returns an executable graph; jh_graph_launch replays it.  Uploads/downloads/frees and
 * profiling must not be issued while capturing, and every buffer and scratch array must already exist
 * (run the recording once eagerly first).  A graph bakes in device pointers and the kernel instantiations chosen at
 * capture time: it stays valid only until a buffer or image it uses is freed, regrown or re-imported, or an eager run
 * makes a scratch array grow.  jh_graph_launch detects this (a generation counter) and returns JH_ERR_INVALID.
 * Two internal counters (flatten's work lists, backdrop's wide-row list) are zeroed by kernels of the frame itself
 * instead of by fill launches, so a captured frame contains no fill for them: it assumes, like every frame, that the
 * frame before it ran to its end.  A stage that fails half-way leaves a host-side flag down: the next eager stage fills
 * again, and jh_graph_launch zeroes the counters its graph has no fill for before it replays (counted:
 * jh_debug_graph_self_cleans). */
int jh_graph_begin(jh_ctx* ctx);
int jh_graph_end(jh_ctx* ctx, void** graph_exec);
int jh_graph_launch(jh_ctx* ctx, void* graph_exec);
/* What the capture recorded: kernel launches and other nodes (fills, copies) of one replay -- the launches per frame. */
int jh_graph_node_counts(jh_ctx* ctx, void* graph_exec, uint32_t* kernel_nodes, uint32_t* other_nodes);
int jh_graph_destroy(jh_ctx* ctx, void* graph_exec);

/* ---- surface blit (RenderToSurface, engine/wgpu_engine/lib.go:266-333) ----
 * The reference renders into an RGBA16F target and then draws it into the surface with a blit pass that premultiplies
 * (vec4(rgb * a, a), lib.go:109-198) and writes RendererOptions.SurfaceFormat (lib.go:19-22).  jh_surface_format is that
 * choice; it is separate from JlImageFormat, which mirrors renderer.ImageFormat.
 *
 * Conversion rule (the hardware's float -> unorm and linear -> sRGB conversions are implementation-defined; this is the
 * project's definition, DESIGN.md "Surface blit"):  c = a colour channel, a = alpha, both the stored f16 widened to f32.
 *   premultiply   p = c * a in f32 (exact: an f16 x f16 product needs at most 22 significand bits); alpha passes as a
 *   clamp         v = min(max(p, 0), 1); NaN (inf * 0 included) -> 0, +inf -> 1
 *   unorm         u8 = rint_f32(v * 255.0f)  (the product rounded to nearest-even in f32, then ties to even) -- also alpha in
 *                 every format
 *   sRGB colour   u8 = rint_f64(255 enc(v)), enc(v) = 12.92 v for v <= 0.0031308, 1.055 v^(1/2.4) - 0.055 otherwise, in
 *                 binary64 on the f32 value; alpha stays linear.  The kernel uses a table of 255 f32 thresholds
 *                 (jello_amd/csrc/srgb_encode_lut.h, tools/gen_srgb_encode_table.py): u8 = #{k : t[k] <= v}
 *   channel order BGRA formats swap bytes 0 and 2 */
typedef enum jh_surface_format {
    JH_SURFACE_RGBA8_UNORM = 0,
    JH_SURFACE_BGRA8_UNORM = 1,
    JH_SURFACE_RGBA8_SRGB = 2,
    JH_SURFACE_BGRA8_SRGB = 3
} jh_surface_format;
/* Converts the RGBA16F image src_image_id (width x height, JL_RGBA16_FLOAT) into caller-owned device memory: height rows of
 * 4 * width bytes, dst_pitch_bytes apart; the bytes between 4 * width and the pitch are never written.  Stream-ordered on the
 * context's stream, one kernel launch, may be captured between jh_graph_begin and jh_graph_end (the graph then holds
 * dst_device_ptr).  A source that was never written (created only, or uploaded as all zero bytes) blits as transparent black.
 * In band mode (jh_set_band) only the pixel rows of the active bin rows are written, so the bands of several contexts compose
 * into one surface.  With profiling on it is a query labelled "blit" with stage = -1 in jh_profile_collect_tree (not a
 * jh_profile_collect record).  JH_ERR_INVALID, with nothing enqueued, for an unknown or non-RGBA16F source, a size that differs
 * from the source's, a pitch below 4 * width, a null dst or an unknown format. */
int jh_blit(jh_ctx* ctx, uint64_t src_image_id, void* dst_device_ptr, uint64_t dst_pitch_bytes, uint32_t width, uint32_t height,
            int surface_format);

/* ---- YUV blit: the RGBA16F target as planar 8-bit Y'CbCr 4:2:0 for a video encoder (DESIGN.md 5.5 "YUV blit") ----
 * The project defines the result byte for byte (tests/yuv_ref.py restates it):
 *   codes     (R, G, B) of a pixel = bytes 0, 1, 2 of what jh_blit writes for it in JH_SURFACE_RGBA8_UNORM (JH_YUV_TRANSFER_NONE)
 *             or JH_SURFACE_RGBA8_SRGB (JH_YUV_TRANSFER_SRGB): premultiplied, clamped, NaN -> 0.  Alpha is dropped: the frame
 *             composited over black.
 *   matrix    in integers, with the coefficient table M (3 x 3, 16.16 fixed point) and the luma offset o of the matrix and range:
 *               Y  = clamp8(o   + floor((M[0] . (R, G, B)       + 2^15) / 2^16))
 *               Cb = clamp8(128 + floor((M[1] . (S_R, S_G, S_B) + 2^17) / 2^18)),  Cr the same with M[2]
 *             S_* = the sum of the codes of the four luma positions the chroma sample covers; floor is towards -inf (an
 *             arithmetic shift); clamp8 is to [0, 255] (it only ever acts on full-range chroma, where 255.5 rounds to 256).
 *   siting    chroma planes are ceil(w / 2) x ceil(h / 2); sample (cx, cy) covers x in {2 cx, min(2 cx + 1, w - 1)} and
 *             y in {2 cy, min(2 cy + 1, h - 1)}: a centre-sited box average (JPEG / MPEG-1), the last column or row counted
 *             twice at an odd edge.
 *   tables    round-half-even(exact * 2^16) of the BT.601 (Kr 0.299, Kb 0.114) and BT.709 (Kr 0.2126, Kb 0.0722) coefficients,
 *             scaled by 219/255 (luma) and 224/255 (chroma) in limited range (o = 16) and by 1 in full range (o = 0); the
 *             green coefficient of a row adjusted so that the Y row sums to rne(scale * 2^16) and each chroma row to 0 -- every
 *             grey has Cb = Cr = 128.  jello_amd/csrc/yuv_matrix_lut.h, tools/gen_yuv_table.py.   (Y row | Cb row | Cr row)
 *               BT.601 limited   16829, 33039, 6416 |  -9714, -19070, 28784 | 28784, -24103, -4681
 *               BT.601 full      19595, 38470, 7471 | -11058, -21710, 32768 | 32768, -27439, -5329
 *               BT.709 limited   11966, 40254, 4064 |  -6596, -22188, 28784 | 28784, -26145, -2639
 *               BT.709 full      13933, 46871, 4732 |  -7509, -25259, 32768 | 32768, -29763, -3005
 *             The result is within 0.51 code of the exact real-valued formula on the same codes.
 *   layouts   NV12: plane[0] = Y (w bytes per row), plane[1] = interleaved (Cb, Cr) pairs (2 ceil(w / 2) bytes per row);
 *             plane[2] is ignored.  I420: plane[0] = Y, plane[1] = Cb, plane[2] = Cr (ceil(w / 2) bytes per row each).
 *             YV12 is I420 with the two chroma pointers swapped. */
typedef enum jh_yuv_layout { JH_YUV_NV12 = 0, JH_YUV_I420 = 1 } jh_yuv_layout;
typedef enum jh_yuv_matrix { JH_YUV_BT601 = 0, JH_YUV_BT709 = 1 } jh_yuv_matrix;
typedef enum jh_yuv_range { JH_YUV_LIMITED = 0, JH_YUV_FULL = 1 } jh_yuv_range;
typedef enum jh_yuv_transfer { JH_YUV_TRANSFER_NONE = 0, JH_YUV_TRANSFER_SRGB = 1 } jh_yuv_transfer;
typedef struct jh_yuv_desc {
    int32_t layout, matrix, range, transfer; /* jh_yuv_layout, jh_yuv_matrix, jh_yuv_range, jh_yuv_transfer */
    void* plane[3];                          /* caller-owned device memory */
    uint64_t pitch[3];                       /* bytes between the rows of each plane */
} jh_yuv_desc;
/* Converts the RGBA16F image src_image_id (width x height, JL_RGBA16_FLOAT) into the planes of *desc (read during the call
 * only).  Any plane pointer and any pitch >= the row's bytes is legal; planes whose pointers and pitches are all multiples of
 * 16 take the kernel's wide stores, everything else single-byte stores of the same bytes.  The bytes between a row's end and
 * the pitch, and the rows below a plane, are never written.  Otherwise as jh_blit: stream-ordered on the context's stream, one
 * kernel launch, may be captured between jh_graph_begin and jh_graph_end (the graph then holds the plane pointers); a source
 * that was never written converts as transparent black (Y = 16 or 0, chroma 128); with profiling on it is a query labelled
 * "blit_yuv" with stage = -1 in jh_profile_collect_tree.  In band mode (jh_set_band) only the luma rows of the active bin rows
 * and the chroma rows under them are written (a bin row is 256 pixel rows, so the cut is even and bands compose).
 * JH_ERR_INVALID, with nothing enqueued, for a null desc, an unknown or non-RGBA16F source, a size that differs from the
 * source's, a null required plane, a pitch below the row's bytes or an unknown layout, matrix, range or transfer. */
int jh_blit_yuv(jh_ctx* ctx, uint64_t src_image_id, uint32_t width, uint32_t height, const jh_yuv_desc* desc);

/* ---- tile-packed frame transport (DESIGN.md 5.4 "Tile pack: the format") ----
 * jh_pack_tiles turns a frame in device memory into only the bytes that have to leave the GPU, jh_unpack_tiles applies such a
 * pack to a frame on the receiving side.  Lossless; the result is defined byte for byte (tests/tilepack_ref.py restates it).
 *
 * A frame is `height` rows of `width` texels of texel_bytes = 4 (an 8-bit surface as jh_blit writes it) or 8 (the RGBA16F
 * target), rows `pitch` bytes apart.  Texels are opaque bit patterns: equal means equal bytes (NaNs and -0 are just patterns).
 * Tiles are 16 x 16 texels, tiles_x = ceil(width / 16), tiles_y = ceil(height / 16), tile index t = ty * tiles_x + tx; only
 * the texels of a tile that lie inside the frame take part in a comparison.  An optional reference frame has the same width,
 * height and texel size and a pitch of its own.  Class of a tile, in this order of precedence:
 *   SKIP   a reference is given and every in-frame texel equals the reference's: nothing is stored
 *   SOLID  all in-frame texels are equal: one texel is stored
 *   RAW    256 texels are stored, row-major inside the tile, texels outside the frame as zero bytes
 * A pack is one byte string:
 *   header   8 x u32, little endian: magic 0x3150544A ("JTP1"), width, height, texel_bytes, n_entries, n_solid, n_raw,
 *            flags (bit 0: a reference was used)
 *   entries  n_entries x (u32 word0, u32 word1), ascending tile index: word0 = t | (RAW ? 1u << 31 : 0), word1 = the index
 *            of the tile's payload within its section (the k-th SOLID entry has k, the k-th RAW entry has k, both from 0)
 *   solid    n_solid texels
 *   raw      n_raw blocks of 256 texels
 * Every section starts at the next multiple of 16 bytes and the padding bytes are zero.  n_entries = n_solid + n_raw, so the
 * total size follows from the header alone:
 *   32 + align16(8 n_entries) + align16(texel_bytes n_solid) + 256 texel_bytes n_raw.
 * jh_pack_bound is the size of the all-RAW pack; no pack is larger (8 bytes per tile, plus the header, over the plain frame
 * rounded up to whole tiles).  Bytes of the destination beyond the pack's total size are never written.
 *
 * Reading a pack (it arrives over a wire: untrusted).  The header is rejected -- the whole pack ignored, counted as one
 * reject -- unless magic, width, height and texel_bytes are the expected ones, n_solid + n_raw = n_entries, n_entries <= the
 * tile count, and the total size <= pack_bytes.  An entry is rejected -- ignored, counted -- when its tile index
 * (word0 & 0x7fffffff) >= the tile count or its word1 >= its section's count.  flags are not interpreted; entries are not
 * required to ascend, and which of two entries with the same tile index wins is unspecified.
 *
 * All pointers are caller-owned device memory (jh_image_device_ptr, jh_buffer_device_ptr, a surface given to jh_blit, another
 * framework's tensor).  Both calls are stream-ordered on the context's stream, read nothing back and never wait; every count
 * stays on the device, so both may be captured between jh_graph_begin and jh_graph_end (frame -> blit -> pack as one graph).
 * Scratch (a byte per tile) comes from the context's arrays and only grows: like a recording, pack a frame of the size once
 * eagerly before capturing.  jh_pack_tiles is two kernel launches, jh_unpack_tiles one.  Band mode (jh_set_band) affects
 * neither call: both always cover the whole frame.  With profiling on each call is a query of its own ("pack", "unpack",
 * stage = -1) in jh_profile_collect_tree, like jh_blit.
 * jh_pack_tiles writes header, entries, payloads and padding; the result is a pure function of its inputs.
 * jh_unpack_tiles writes the in-frame texels of the accepted SOLID and RAW entries into dst and touches nothing else: not the
 * SKIP tiles, not the bytes between width * texel_bytes and the pitch, not the rows below the frame.  It never reads outside
 * [pack, pack + pack_bytes) or writes outside the frame, whatever the bytes are.
 * JH_ERR_INVALID, with nothing enqueued: a null src / dst / pack, a texel size other than 4 or 8, width or height 0 (or more than
 * 2^31 - 1 tiles), a pitch below width * texel_bytes, a pointer or pitch that is not a multiple of texel_bytes,
 * dst_capacity < jh_pack_bound(...), pack_bytes < 32.  Any other alignment works (a pitch of 4 * width + 4 is legal); the
 * 16-byte accesses of the fast path need pointers and pitches that are multiples of 16. */
uint64_t jh_pack_bound(uint32_t width, uint32_t height, uint32_t texel_bytes); /* 0 for a bad texel size */
int jh_pack_tiles(jh_ctx* ctx, const void* src, uint64_t src_pitch, const void* ref /* or NULL */, uint64_t ref_pitch, uint32_t width,
                  uint32_t height, uint32_t texel_bytes, void* dst, uint64_t dst_capacity);
int jh_unpack_tiles(jh_ctx* ctx, const void* pack, uint64_t pack_bytes, void* dst, uint64_t dst_pitch, uint32_t width, uint32_t height,
                    uint32_t texel_bytes);
/* What jh_unpack_tiles has rejected since the last reset (entries; a rejected header counts once).  Synchronises the stream. */
int jh_debug_unpack_rejects(jh_ctx* ctx, uint32_t* count, int reset);

/* ---- dashing (DESIGN.md 5.6 "Dash rule") ----
 * jh_dash turns a batch of paths into their dashes on the device: for callers that dash many paths per frame (the host route,
 * Scene.stroke with a pattern, does the same on one core).  The result is defined word for word by the rule of DESIGN.md 5.6,
 * stated in include/jello_dash.h -- which the host route compiles too -- and restated by tests/dash_ref.py; all three agree
 * byte for byte.  The rule in short: dashing happens in user space; pattern entries, the offset and every segment's length are
 * quantised once to 2^-20 user units and every position along a subpath is an integer sum; the pattern alternates on / off
 * starting with on (an odd one keeps alternating, its period is two cycles), every subpath starts again at the offset, "on"
 * intervals are half open, a zero "on" emits nothing and a zero "off" joins its neighbours; a dash is MoveTo(its start) + one
 * sub-curve of the source's kind per segment it overlaps, cut by de Casteljau in binary64 and rounded once to binary32, with
 * the source's control points copied where a cut falls on a segment's end; a closed subpath's last and first dash are one
 * dash when they meet at its start (emitted last), and one dash that covers a closed subpath is closed with ClosePath.
 *
 * Input, host memory, read during the call only:
 *   els      the elements of all paths: {i32 kind (0 MoveTo, 1 LineTo, 2 QuadTo, 3 CubicTo, 4 ClosePath), i32 pad, f64 pts[6]}
 *   paths    per path {u32 first_el, n_els, first_dash, n_dash; f64 offset}: its elements, and its pattern in `dashes`
 *   dashes   the concatenated patterns
 * Output, caller-owned device memory:
 *   out_els    out_capacity elements {u32 kind, f32 p[6]} (28 bytes): path after path, subpath after subpath, dash by ascending
 *              start (a merged one last), segment after segment inside a dash
 *   out_index  n_paths + 1 words: the exclusive offset of every path's elements, the last word = the total the job needs
 * Elements at or beyond out_capacity are not written, the total still reports the need: read it, regrow, call again (the
 * pipeline's clean-failure-and-regrow convention).  Bytes beyond out_capacity elements are never touched.
 *
 * The job is copied through the pinned staging arena like jh_upload's data; the call is stream-ordered on the context's stream
 * and never waits for the device.  Its grids depend on the job, so it is refused during graph capture.  Scratch comes from the
 * context's arrays (slots A-E, kcommon.h) and only grows.  Seven kernel launches.  With profiling on the call is a query "dash"
 * with stage = -1 in jh_profile_collect_tree.
 * JH_ERR_INVALID, with nothing enqueued and nothing written: a null pointer; a pattern with 0 or more than 64 entries; an entry
 * that is negative, not finite or above 2^30; a quantised period of 0; an offset that is not finite or beyond 2^40 in magnitude;
 * a coordinate that is not finite or beyond 2^20 in magnitude; an unknown element kind; a path whose elements or pattern lie
 * outside the arrays; more than 2^31 - 1 drawn segments; out_capacity above 2^32 - 1.  The totals are 32-bit words: a job whose
 * output would pass 2^32 - 1 elements writes nothing out of bounds but its index is meaningless. */
typedef struct jh_dash_el { int32_t kind, pad; double pts[6]; } jh_dash_el;
typedef struct jh_dash_path { uint32_t first_el, n_els, first_dash, n_dash; double offset; } jh_dash_path;
typedef struct jh_dash_out_el { uint32_t kind; float p[6]; } jh_dash_out_el;
int jh_dash(jh_ctx* ctx, const jh_dash_el* els, uint64_t n_els, const jh_dash_path* paths, uint32_t n_paths, const double* dashes,
            uint64_t n_dashes, void* out_els, uint64_t out_capacity, uint32_t* out_index);

/* ---- Gaussian blur of an RGBA16F image (DESIGN.md 5.7 "Blur rule") ----
 * Drop shadows, glows, backdrop blur, feGaussianBlur and CSS blur() without the target leaving the device.  The result is defined
 * on values, not on passes, and every implementation produces these bits (include/jello_blur.h states the host half,
 * tests/blur_ref.py restates all of it):
 *   taps        one axis with standard deviation sigma (binary32, used as binary64), 0 <= sigma <= 64 = JH_BLUR_MAX_SIGMA:
 *               R = ceil(3 sigma) <= 192; sigma = 0: R = 0 and the single tap 1.0f; otherwise g_k = exp(-(double)(k k) / (2.0 sigma
 *               sigma)), k = 0..R (one libm exp per tap, the only inexact library call), S = g_0 + 2 (g_1 + ... + g_R) with the
 *               bracket summed in that order in binary64, w_k = (float)(g_k / S), w_-k = w_k.
 *   horizontal  per texel and channel  H = 0.0f; for k = -R_x .. +R_x ascending: H = fmaf(w_k, (float)src[x + k], H)
 *               -- a fused multiply-add; H is binary32 and is never rounded to f16.
 *   vertical    V = 0.0f; for k = -R_y .. +R_y ascending: V = fmaf(w_k, H[y + k], V); dst = f16(V), round to nearest even, once.
 *   edges       JH_BLUR_EDGE_ZERO: a tap outside the image contributes nothing (its fmaf is not executed);
 *               JH_BLUR_EDGE_CLAMP: it reads the nearest texel of the image.  The image is the edge, not the rectangle.
 *   values      f16 subnormals are values, in and out: nothing is flushed.  Inf and NaN follow IEEE; a NaN result is any NaN.
 * So sigma_x = sigma_y = 0 is a bit-exact copy of every value (a -0 comes out as +0: fmaf(1, -0, +0) = +0; a NaN as a NaN), and
 * sigma = 0 on one axis leaves the one rounding of the other axis' sum.
 *
 * jh_blur_taps: the 2R + 1 taps of `sigma` into weights (weights[k + R] = w_k; may be NULL) and R into *radius (may be NULL).
 * Host only, no context.  JH_ERR_INVALID for a sigma that is negative, above 64 or NaN.
 *
 * jh_blur: blurs the image src_image_id (width x height, JL_RGBA16_FLOAT) into the rectangle (x, y, width, height) of
 * dst_image_id (the same size and format); desc->width == desc->height == 0 means the whole image (x and y are then ignored).
 * dst_image_id may equal src_image_id: in place, with the result of a blur into a second image.  Texels of dst outside the
 * rectangle keep their bits; a dst that was never written is cleared to transparent black first, so outside the rectangle it
 * reads as it did before; dst then counts as written.  Source texels outside the rectangle but inside the image take part with
 * their real values; a source that was never written reads as transparent black.
 * Stream-ordered on the context's stream, never waits: two kernel launches (rows into a binary32 intermediate, columns out of
 * it), plus a fill when dst has to be cleared.  The intermediate lives in a scratch array of the context, at most
 * (rect height + 2 R_y) x rect width x 16 bytes, which only grows: the call may be captured between jh_graph_begin and
 * jh_graph_end once a rectangle of this size has been blurred eagerly (a capture that would have to grow it is refused with
 * JH_ERR_OOM and that advice).  With profiling on the call is a query "blur" with stage = -1 in jh_profile_collect_tree.
 * Not in band mode (jh_set_band): the rows next to a band belong to another rank's context, and a blur reads across them.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_blur: ": a null
 * desc; an unknown source or destination id; an image that is not RGBA16F or whose size differs from width x height; a sigma that
 * is negative, above 64 or NaN; an unknown edge mode; a rectangle that is not inside the image or that is empty in exactly one
 * dimension; a band set with jh_set_band. */
#define JH_BLUR_MAX_SIGMA 64.0f
typedef enum jh_blur_edge { JH_BLUR_EDGE_ZERO = 0, JH_BLUR_EDGE_CLAMP = 1 } jh_blur_edge;
typedef struct jh_blur_desc {
    float sigma_x, sigma_y;
    int edge;                     /* JH_BLUR_EDGE_ZERO | JH_BLUR_EDGE_CLAMP */
    uint32_t x, y, width, height; /* rectangle of dst that is written; width == height == 0: the whole image */
} jh_blur_desc;
int jh_blur_taps(float sigma, float* weights /* 2R+1 entries, or NULL */, uint32_t* radius);
int jh_blur(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, uint32_t width, uint32_t height, const jh_blur_desc* desc);

/* ---- Composite: one RGBA16F image blended onto another (DESIGN.md 5.8 "Composite rule") ----
 * What a blurred layer needs to become a drop shadow, a glow or an overlay without leaving the device: a rectangle of the image
 * src_image_id is blended onto dst_image_id with any of the 16 mix modes x 14 Porter-Duff operators, an opacity and an optional
 * tint.  The images are stored un-premultiplied (as fine stores them), and may differ in size.  The result is defined on values
 * (include/jello_composite.h states the geometry, jello_amd/csrc/blend_rule.h the blend, tests/composite_ref.py restates all of
 * it); per texel of the written rectangle, all in binary32, every operation rounded once, nothing contracted:
 *   source      (c_s, a_s) = the f16 texel widened.  With JH_COMPOSITE_TINT: c_s = tint.rgb (binary32 as given) and
 *               a_s = a_s * tint.a.  Then a_s = a_s * opacity, and p_s = c_s * a_s.  (No tint and opacity 1: every step is exact.)
 *   backdrop    (c_b, a_b) = the dst texel widened, p_b = c_b * a_b (exact).  A dst that was never written reads as transparent black.
 *   blend       R = blend_mix_compose((p_b, a_b), (p_s, a_s), mix << 8 | compose): the function the fine stage applies at END_CLIP
 *               (shared/blend.wgsl), operation for operation, with its fast arm for Normal + SrcOver (R = p_b * (1 - a_s) + p_s, also
 *               for alpha) and EPSILON = 1e-15f.  Its min / max are IEEE minNum / maxNum (a NaN operand yields the other one) with
 *               -0 below +0.
 *   store       as fine does: a_inv = 1.0f / max(R.a, 1e-6f); dst = (f16(R.r * a_inv + 0.0f), f16(R.g * a_inv + 0.0f),
 *               f16(R.b * a_inv + 0.0f), f16(R.a + 0.0f)), round to nearest even.  The + 0.0f turns a binary32 -0 into +0.
 *               A NaN result is any NaN; f16 subnormals are values, nothing is flushed.
 * Consequences: opacity 0, or a transparent source, under Normal + SrcOver gives back every dst texel with a_b >= 1e-6 bit for bit
 * (a -0 as +0); the colour of a dst texel with a_b = 0 becomes 0; Compose.Clear (compose = 3) clears the
 * rectangle.  Outside the placed rectangle nothing is ever written, also by operators that would erase the backdrop where the
 * source is absent (SrcIn, Copy, ...): the layer is its rectangle.
 *
 * Geometry: the source rectangle (sx, sy, sw, sh) must lie inside the source image; sw == sh == 0 means the whole image (sx, sy
 * ignored).  Its top-left lands at the signed (dx, dy) of dst and it is clipped to dst; a placement that clips to nothing is
 * JH_OK and launches nothing.
 * Stream-ordered on the context's stream, never waits: one kernel launch (plus a fill when a never-written dst has to be cleared:
 * it is cleared first when the placed rectangle is not the whole image, and counts as written afterwards).  No scratch, a fixed
 * grid: the call may always be captured between jh_graph_begin and jh_graph_end.  With profiling on it is a query "composite" with
 * stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band): a shifted source row belongs to another rank.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_composite: ":
 * a null desc; an unknown source or destination id; an image that is not RGBA16F; src == dst (a shifted blend in place reads what
 * it writes); mix > 15 (so Mix.Clip); compose > 13; an opacity or a tint alpha outside [0, 1] or NaN; a tint colour that is not
 * finite; unknown flag bits; a source rectangle that is not inside the source image or that is empty in exactly one dimension; a
 * band set with jh_set_band.  (The tint is read only with the flag.) */
#define JH_COMPOSITE_TINT 1u
typedef struct jh_composite_desc {
    uint32_t mix, compose;          /* Mix 0..15, Compose 0..13 (the encodings of gfx.h / scene.py) */
    float opacity;                  /* [0, 1] */
    uint32_t flags;                 /* bit 0: JH_COMPOSITE_TINT */
    float tint[4];                  /* r, g, b finite; a in [0, 1]; read only with the flag */
    uint32_t sx, sy, sw, sh;        /* source rectangle; sw == sh == 0: the whole source */
    int32_t dx, dy;                 /* where its top-left lands in dst */
} jh_composite_desc;
int jh_composite(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_composite_desc* desc);

/* ---- Resample: one RGBA16F image resized into a rectangle of another (DESIGN.md 5.9 "Resample rule") ----
 * A 4096^2 render as a 1080p video frame, a supersampled render at display size, thumbnails, mip levels, a layer scaled before
 * jh_composite places it -- without the image leaving the device.  The result is defined on values, and every implementation
 * produces these bits (include/jello_resample.h states the host half, tests/resample_ref.py restates all of it).
 * Per axis, with n_in the SOURCE RECTANGLE's extent and n_out the destination rectangle's, binary64 unless said otherwise:
 *   support     scale = (double)n_in / (double)n_out; fs = max(scale, 1.0); support = base fs, base = 0.5 BOX, 1.0 TRIANGLE,
 *               2.0 CATMULL_ROM, 3.0 LANCZOS3.  Legal: n_in >= 1, n_out >= 1, n_in <= 16 n_out (16:1 down at most, any ratio up).
 *   window      of output i: c = ((double)i + 0.5) scale; lo = max(0, (int64)(c - support + 0.5)); hi = min(n_in, (int64)(c +
 *               support + 0.5)), the casts truncating.  It is clipped to the source rectangle, not to the image: an atlas cell
 *               does not bleed.  g_k = f(((double)k - c + 0.5) / fs), k = lo .. hi - 1; leading and trailing g_k that are exactly
 *               0.0 are dropped, interior zeros stay.  No window is empty, none has more than 96 taps.
 *   filters     operations in this order -- BOX: 1.0 if -0.5 < x <= 0.5, else 0.0.  TRIANGLE: x = |x|; 1.0 - x if x < 1.0, else 0.0.
 *               CATMULL_ROM: a = -0.5, x = |x|; ((a + 2.0) x - (a + 3.0)) x x + 1.0 if x < 1.0; (((x - 5.0) x + 8.0) x - 4.0) a if
 *               x < 2.0; else 0.0.  LANCZOS3: sinc(x) sinc(x / 3.0) if -3.0 <= x < 3.0, else 0.0; sinc(0) = 1, otherwise t = x M_PI,
 *               sin(t) / t -- sin is the libm call, the rule's only inexact library call.
 *   taps        S = the sum of the window's g_k, ascending k; w_k = (float)(g_k / S).
 * Per texel, binary32, nothing contracted but the stated fmaf:
 *   source      the f16 texel widened to (c, a); p = (c.r a, c.g a, c.b a, a), exact -- or with JH_RESAMPLE_STRAIGHT p = (c, a), for
 *               data images and constant alpha.  (The images are stored un-premultiplied, DESIGN.md 5.8: filtering their colour
 *               channels is right only where alpha is constant, so premultiplying is the default.)
 *   horizontal  H = 0.0f; for k ascending over the x window: H = fmaf(w_k, p[k], H).  H stays binary32.
 *   vertical    V = 0.0f; for k ascending over the y window: V = fmaf(w_k, H[k], V).  Rows before columns: the bits depend on it.
 *   store       STRAIGHT: f16(V) per channel, round to nearest even.  Otherwise as fine and jh_composite store: a_inv = 1.0f /
 *               max(V.a, 1e-6f); (f16(V.r a_inv + 0.0f), f16(V.g a_inv + 0.0f), f16(V.b a_inv + 0.0f), f16(V.a + 0.0f)).
 *   values      f16 subnormals are values, Inf and NaN follow IEEE, a NaN result is any NaN.  Nothing is clamped: the negative lobes
 *               of CATMULL_ROM and LANCZOS3 can leave alpha below 0 or colour above 1.
 * So STRAIGHT with equal sizes is a bit-exact copy under BOX, TRIANGLE and CATMULL_ROM (the single tap 1.0f; a -0 comes out as +0,
 * a NaN as a NaN) -- not under LANCZOS3, because sin(k pi) is not 0 in binary64 -- and STRAIGHT BOX at an exact 2:1 is the 2 x 2
 * mean with the rule's roundings.
 *
 * jh_resample_taps: the window of output i of an axis: its weights into weights (96 entries are enough; may be NULL), its first
 * source index (relative to the source rectangle) into *first and its tap count into *count (either may be NULL).  Host only, no
 * context.  JH_ERR_INVALID for an unknown filter, illegal sizes or i >= n_out.
 *
 * jh_resample: the rectangle (src_x, src_y, src_width, src_height) of src_image_id resized into the rectangle (dst_x, dst_y,
 * dst_width, dst_height) of dst_image_id, another image; the images carry their own sizes; width == height == 0 means the whole
 * image (x and y are then ignored).  Only the destination rectangle is written; a dst that was never written is cleared to
 * transparent black first and then counts as written; a source that was never written reads as transparent black.
 * Stream-ordered on the context's stream, never waits: two kernel launches (rows into a binary32 intermediate of source-rectangle
 * rows x dst_width x 16 bytes, columns out of it), plus a fill when dst has to be cleared.  The windows and taps of both axes live in
 * a device table of the context, which holds ONE geometry (filter and the four extents) at a time: a call with the geometry the
 * table holds uploads nothing; an eager call with another builds the tables on the host, uploads them stream-ordered and makes every
 * graph captured before it stale (jh_graph_launch refuses it).  During a capture a call whose geometry is resident records its two
 * launches; any other is refused with JH_ERR_OOM and the advice to resample this geometry once eagerly first.  With profiling on the
 * call is a query "resample" with stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band).
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_resample: ": a
 * null desc; an unknown source or destination id; an image that is not RGBA16F; an unknown filter or flag bit; a rectangle that is
 * not inside its image or that is empty in exactly one dimension; a ratio above 16:1 on either axis; src_image_id == dst_image_id; a
 * band set with jh_set_band. */
typedef enum jh_resample_filter { JH_RESAMPLE_BOX = 0, JH_RESAMPLE_TRIANGLE = 1, JH_RESAMPLE_CATMULL_ROM = 2, JH_RESAMPLE_LANCZOS3 = 3 } jh_resample_filter;
#define JH_RESAMPLE_STRAIGHT 1u
#define JH_RESAMPLE_MAX_TAPS 96u
typedef struct jh_resample_desc {
    int filter;                                       /* jh_resample_filter */
    uint32_t flags;                                   /* bit 0: JH_RESAMPLE_STRAIGHT */
    uint32_t src_x, src_y, src_width, src_height;     /* source rectangle; width == height == 0: the whole image */
    uint32_t dst_x, dst_y, dst_width, dst_height;     /* destination rectangle, likewise */
} jh_resample_desc;
int jh_resample_taps(int filter, uint32_t n_in, uint32_t n_out, uint32_t i, float* weights /* or NULL */, uint32_t* first, uint32_t* count);
int jh_resample(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_resample_desc* desc);

/* ---- Colour filter: a colour matrix and per-channel transfer functions on an RGBA16F image (DESIGN.md 5.10 "Colour-filter rule") ----
 * feColorMatrix, feComponentTransfer, the CSS filter functions (grayscale, sepia, saturate, hue-rotate, invert, opacity, brightness,
 * contrast), a tint, a luminance mask's first half -- without the image leaving the device.  The result is defined on values, and
 * every implementation produces these bits (include/jello_color.h states the host half, tests/color_ref.py restates all of it).
 * Per texel, binary32, nothing contracted but the stated fmaf; h_c is the stored f16 bit pattern of channel c, un-premultiplied:
 *   input    t_c = PRE_c[h_c] for c = r, g, b when space == JH_COLOR_SRGB; otherwise, and always for alpha, t_c = h_c widened (exact).
 *   matrix   for each output channel i: m = M[i][4]; then m = fmaf(M[i][k], t_k, m) for k = 0, 1, 2, 3 in that order (M = matrix,
 *            row-major 4 x 5, acting on (r, g, b, a, 1): what feColorMatrix is defined on).  THE ORDER IS STATED HERE: the offset
 *            first, then r, g, b, a.  0 x Inf is NaN: a texel with an infinite channel makes every row NaN that multiplies it by 0.
 *   clamp    with JH_COLOR_CLAMP: m = m > 0 ? m : 0, then m = m < 1 ? m : 1 -- compare and select, which sends NaN and -0 to +0.
 *   round    g = f16(m), round to nearest even, a NaN m gives 0x7e00.  The only rounding to f16 on the device.
 *   output   out_i = POST_i[g] where channel i has a table, otherwise out_i = g.
 * The tables have one entry per f16 bit pattern and are built on the host in binary64 (x: the value of the index pattern):
 *   enc      a = |x|; 12.92 a if a <= 0.0031308, else 1.055 pow(a, 1.0 / 2.4) - 0.055; with x's sign (DESIGN.md 5.3's curve extended
 *            odd; +-0 keep their sign, +-Inf give +-Inf).  dec: a = |x|; a / 12.92 if a <= 0.04045, else pow((a + 0.055) / 1.055,
 *            2.4); with x's sign.  pow is the libm call, the rule's only inexact library call, and never runs on the device.
 *   PRE_c    (float)enc(x), in SRGB space only; a NaN x gives the binary32 NaN 0x7fc00000.  Alpha is never encoded.
 *   func_i   IDENTITY x; LINEAR slope x + intercept; GAMMA amplitude pow(x, exponent) + offset; TABLE over n values v_0 .. v_n-1
 *            with N = n - 1: v_0 if N = 0, else c = x > 0 ? x : 0, c = c < 1 ? c : 1, k = min((int)(c N), N - 1), v_k + ((x - k / N)
 *            N) (v_k+1 - v_k) (Filter Effects' formula; the input is clamped for the index only, so outside [0, 1] the first and the
 *            last segment go on); DISCRETE: the same c, k = min((int)(c n), n - 1), v_k.  Parameters are binary32, widened.
 *   POST_i   y = func_i(x); with JH_COLOR_CLAMP y = y > 0 ? y : 0, y = y < 1 ? y : 1; in SRGB space and for i = r, g, b y = dec(y);
 *            the entry is f16(y), rounded once from binary64; a NaN y and every NaN x give 0x7e00.
 *   exists   PRE_c in SRGB space; POST_i where func_i is not IDENTITY or dec applies -- a channel whose composition is the
 *            identity has no table.
 * So in LINEAR space with IDENTITY funcs and no clamp the identity matrix returns a texel of finite channels unchanged except that
 * -0 comes out as +0 (m starts at the offset +0); a NaN comes out as 0x7e00, and an infinite channel survives itself and makes the
 * other three NaN.  In SRGB space the identity is not exact (DESIGN.md 5.10 has the largest deviation).
 *
 * jh_color_tables: the tables of desc (its rectangle and matrix are not looked at): PRE_c into pre[c * 65536 ..], POST_i into
 * post[i * 65536 ..] for the tables that exist -- the entries of the others are left alone -- and into *which bit c for PRE_c and
 * bit 4 + i for POST_i; each pointer may be NULL.  Host only, no context.  JH_ERR_INVALID for a null desc, an unknown space, func
 * type or flag bit, n = 0 or n > 64 values, or a parameter that is not finite (only the parameters a func's type uses are read).
 *
 * jh_color_filter: the rule applied to the rectangle (x, y, width, height) of src_image_id, written to the same rectangle of
 * dst_image_id; width == height == 0 means the whole image (which then has to fit into the other one too).  src == dst is legal: the
 * rule is per texel.  Only the rectangle is written; a dst that was never written is cleared to transparent black first and then
 * counts as written; a source that was never written reads as transparent black (and so gives the matrix's offsets).
 * Stream-ordered on the context's stream, never waits: one kernel launch, plus a fill when dst has to be cleared.  A descriptor that
 * needs no tables (LINEAR space, IDENTITY funcs) touches no scratch and is always capturable.  Otherwise the tables live in a device
 * slot of the context, which holds the tables of ONE key (space, clamp bit, the four funcs with the values their types use; the
 * matrix is a kernel argument and no part of it) at a time: a call with the resident key uploads nothing; an eager call with another
 * builds the tables on the host, uploads them stream-ordered and makes every graph captured before it stale (jh_graph_launch refuses
 * it).  During a capture a call whose key is resident records its launch; any other is refused with JH_ERR_OOM and the advice to
 * run this filter once eagerly first.  jh_scratch_trim forgets the key.  With profiling on the call is a query "color" with
 * stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band).
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts
 * "jh_color_filter: ": a null desc; an unknown source or destination id; an image that is not RGBA16F; what jh_color_tables refuses;
 * a matrix entry that is not finite; a rectangle that is not inside both images or that is empty in exactly one dimension; a band
 * set with jh_set_band. */
typedef enum jh_color_space { JH_COLOR_LINEAR = 0, JH_COLOR_SRGB = 1 } jh_color_space;
typedef enum jh_color_func_type {
    JH_COLOR_FUNC_IDENTITY = 0, JH_COLOR_FUNC_LINEAR = 1, JH_COLOR_FUNC_GAMMA = 2, JH_COLOR_FUNC_TABLE = 3, JH_COLOR_FUNC_DISCRETE = 4
} jh_color_func_type;
#define JH_COLOR_CLAMP 1u
#define JH_COLOR_MAX_VALUES 64u
#define JH_COLOR_TABLE_ENTRIES 65536u
typedef struct jh_color_func {
    int type;                                  /* jh_color_func_type */
    uint32_t n;                                /* TABLE, DISCRETE: the count of values, 1 .. 64 */
    float slope, intercept;                    /* LINEAR */
    float amplitude, exponent, offset;         /* GAMMA */
    float values[JH_COLOR_MAX_VALUES];         /* TABLE, DISCRETE */
} jh_color_func;
typedef struct jh_color_desc {
    uint32_t x, y, width, height;              /* the rectangle, in both images; width == height == 0: the whole image */
    float matrix[20];                          /* row-major 4 x 5 on (r, g, b, a, 1) */
    int space;                                 /* jh_color_space */
    uint32_t flags;                            /* bit 0: JH_COLOR_CLAMP */
    jh_color_func func[4];                     /* per output channel r, g, b, a, applied after the matrix */
} jh_color_desc;
int jh_color_tables(const jh_color_desc* desc, float* pre /* 3 x 65536 or NULL */, uint16_t* post /* 4 x 65536 or NULL */, uint32_t* which);
int jh_color_filter(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_color_desc* desc);

/* ---- Morphology: erode and dilate of an RGBA16F image by a box (DESIGN.md 5.11 "Morphology rule") ----
 * A shadow with spread, an outline or halo around text, a matte choked before compositing, opening and closing a mask,
 * feMorphology -- without the image leaving the device.  The result is defined on values, and every implementation produces these
 * bits (include/jello_morph.h states the host half and the order key, tests/morph_ref.py restates all of it).
 *   arguments   op: JH_MORPH_ERODE = 0 | JH_MORPH_DILATE = 1.  radius_x, radius_y: integers in [0, JH_MORPH_MAX_RADIUS = 255].
 *               edge: JH_MORPH_EDGE_ZERO = 0 | JH_MORPH_EDGE_CLAMP = 1.  flags: bit 0, JH_MORPH_STRAIGHT.  The rectangle (x, y, width,
 *               height) of dst is written; width == height == 0 means the whole image (x and y are then ignored).
 *   operand     the f16 texel widened to binary32 (c, a); p = (c.r a, c.g a, c.b a, a), each product of two f16 values exact in
 *               binary32: the premultiplied colour feMorphology is defined on.  With JH_MORPH_STRAIGHT p = (c, a) as stored, for
 *               data images and masks.
 *   window      output texel (X, Y) of the rectangle takes the image positions [X - rx, X + rx] x [Y - ry, Y + ry], the box
 *               structuring element of feMorphology.  The IMAGE is the edge, not the rectangle: source texels outside the rectangle
 *               but inside the image take part with their real values.  A position outside the image: EDGE_ZERO: it takes part as
 *               transparent black, +0.0f in all four channels (an erode eats the shape at the image's border, as the specification
 *               has it); EDGE_CLAMP: it does not take part -- the window is clipped to the image, which is what reading the nearest
 *               texel gives for an idempotent operator.  A source that was never written reads as transparent black.
 *   order       per channel, independently, on binary32.  If any operand of the window is a NaN (either sign) the result is a NaN.
 *               Otherwise DILATE is the greatest and ERODE the least operand in IEEE 754 totalOrder (-Inf < ... < -0 < +0 < ... <
 *               +Inf; -0 and +0 are different values and +0 is the greater).  As integer keys: k = bits ^ ((int32)bits >> 31 &
 *               0x7fffffff) compared as signed, a NaN mapped to the extreme the operator selects.  Nothing else is computed: the
 *               result is one of the operands, no rounding occurs and no evaluation order has to be fixed.  THE RESULT IS DEFINED ON
 *               THE WINDOW, NOT ON PASSES: rows then columns, block prefix / suffix extrema and doubling all give these bits, and
 *               the implementation is free to choose.
 *   store       STRAIGHT: f16(V) per channel, exact (V is a widened f16).  Otherwise as fine, jh_composite and jh_resample store:
 *               a_inv = 1.0f / max(V.a, 1e-6f); (f16(V.r a_inv + 0.0f), f16(V.g a_inv + 0.0f), f16(V.b a_inv + 0.0f), f16(V.a +
 *               0.0f)), round to nearest even.
 *   values      f16 subnormals are values, in and out.  Inf x 0 in the premultiply is a NaN and propagates.  A NaN result is any NaN.
 * So STRAIGHT with rx = ry = 0 is a bit-exact copy of every non-NaN value, -0 included (unlike the blur); without STRAIGHT radius 0
 * leaves the store's rounding of c a / a.  STRAIGHT erode equals the sign-flipped dilate of the sign-flipped image: exactly under
 * CLAMP; under ZERO the flipped route pads with -0 seen from the original, so the two differ exactly in the channels whose window
 * reaches outside the image and holds no operand below +0 inside it -- erode gives +0 there (the padding), the flipped route -0 --
 * and nowhere else.  Under CLAMP dilate >= source >= erode in the order, texel by texel; on values (STRAIGHT) both are the identity
 * at radius 0, hence idempotent there, and monotone in the radius; erode by r then dilate by r never exceeds the source.
 *
 * jh_morphology: the rule applied to src_image_id, written to the rectangle of dst_image_id.  The images carry their own sizes and
 * must be JL_RGBA16_FLOAT and of equal size.  dst_image_id may equal src_image_id: in place, with the result of the call into a
 * second image (no pass reads what the call has written).  Texels of dst outside the rectangle keep their bits; a dst that was never
 * written is cleared to transparent black first and then counts as written.
 * Stream-ordered on the context's stream, never waits: THREE kernel launches (rows into a plane of keys; the block prefix of its
 * columns into a second plane; the block suffix, the combination and the store), plus a fill when dst has to be cleared.  None of
 * them walks a window: the cost per texel does not grow with the radius beyond the row pass's log2(2 rx + 1) doubling steps.  The
 * two planes live in a scratch array of the context, 2 x (rect height + 2 radius_y) x rect width x 16 bytes, which only grows: the
 * call may be captured between jh_graph_begin and jh_graph_end once a call of this rectangle size and these radii has run eagerly (a
 * capture that would have to grow it is refused with JH_ERR_OOM and that advice).  With profiling on the call is a query
 * "morphology" with stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band): the rows next to a band belong to
 * another rank's context.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_morphology: ": a
 * null desc; an unknown source or destination id; an image that is not RGBA16F; images of different size; an unknown op, edge or flag
 * bit; a radius above 255; a rectangle that is not inside the image or that is empty in exactly one dimension; a band set with
 * jh_set_band. */
typedef enum jh_morph_op { JH_MORPH_ERODE = 0, JH_MORPH_DILATE = 1 } jh_morph_op;
typedef enum jh_morph_edge { JH_MORPH_EDGE_ZERO = 0, JH_MORPH_EDGE_CLAMP = 1 } jh_morph_edge;
#define JH_MORPH_STRAIGHT 1u
#define JH_MORPH_MAX_RADIUS 255u
typedef struct jh_morph_desc {
    int op;                        /* jh_morph_op */
    int edge;                      /* jh_morph_edge */
    uint32_t flags;                /* bit 0: JH_MORPH_STRAIGHT */
    uint32_t radius_x, radius_y;
    uint32_t x, y, width, height;  /* rectangle of dst that is written; 0 x 0: the whole image */
} jh_morph_desc;
int jh_morphology(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_morph_desc* desc);

/* ---- Warp: an affine transform of a rectangle of one RGBA16F image into a rectangle of another (DESIGN.md 5.12 "Warp rule") ----
 * A rotated, skewed or sub-texel-translated layer, sprite or glyph run, a CSS transform on a filtered layer, a skewed shadow, a tiled
 * pattern (feTile) under REPEAT -- without the image leaving the device.  The result is defined on values, and every implementation
 * produces these bits (include/jello_warp.h states the host half, tests/warp_ref.py restates all of it).
 *   arguments   matrix[6], binary64, in the order the Scene transforms use: (a, b, c, d, e, f), x' = a x + c y + e, y' = b x + d y +
 *               f.  It maps continuous coordinates of the SOURCE RECTANGLE (origin its top-left corner, texel (i, j) centred at
 *               (i + 0.5, j + 0.5)) to continuous coordinates of the DESTINATION IMAGE, not of the destination rectangle: the
 *               destination rectangle is only what gets written, so a warp written in four quadrant rectangles equals the
 *               whole-image warp.  A rectangle of 0 x 0 means the whole image (x and y are then ignored).  filter: JH_WARP_NEAREST
 *               = 0 | JH_WARP_BILINEAR = 1 | JH_WARP_BICUBIC = 2 (Catmull-Rom).  edge: JH_WARP_EDGE_ZERO = 0 | _CLAMP = 1 | _REPEAT
 *               = 2 | _MIRROR = 3.  flags: bit 0, JH_WARP_STRAIGHT.
 *   inverse     binary64, nothing contracted, every product and quotient rounded once: det = a d - b c; p = d / det, q = -c / det,
 *               r = (c f - d e) / det; s = -b / det, t = a / det, w = (b e - a f) / det.  u = p x' + q y' + r, v = s x' + t y' + w.
 *   legal       all six entries finite; det finite and not 0; |p|, |q|, |s|, |t| <= 64; |r|, |w| <= 2^22; both images at most 32768
 *               on a side.  With these limits every integer below stays under 2^58.
 *   plan        six int64: P = rint(p 2^31), likewise Q, S, T; R = rint(r 2^32), likewise W; rint rounds half to even.  For the
 *               destination texel (X, Y) of the image: U = P (2 X + 1) + Q (2 Y + 1) + R, V = S (2 X + 1) + T (2 Y + 1) + W, both
 *               exact: the source position in units of 2^-32 texel.  The device computes exactly these integers.
 *   taps        per axis, on U (V likewise).  NEAREST: one tap at i = U >> 32 (an arithmetic shift: a floor), weight 1.0f.
 *               BILINEAR: U' = U - 2^31, i0 = U' >> 32, k = (U' >> 16) & 0xffff (the low 16 bits are dropped, not rounded), f =
 *               (float)k 2^-16 (exact); taps i0, i0 + 1 with weights 1.0f - f, f (both exact).  BICUBIC: the same i0 and f; taps
 *               i0 - 1 .. i0 + 2; weights in binary32 with these fmaf's and single multiplications:
 *                 w0 = fmaf(fmaf(-0.5f, f, 1.0f), f, -0.5f) f        w1 = fmaf(fmaf(1.5f, f, -2.5f) f, f, 1.0f)
 *                 w2 = fmaf(fmaf(-1.5f, f, 2.0f), f, 0.5f) f         w3 = (fmaf(0.5f, f, -0.5f) f) f
 *   edge        a tap index i is resolved against the source RECTANGLE's extent n (the rectangle is the edge, not the image: an atlas
 *               cell does not bleed).  ZERO: outside [0, n) the operand is +0.0f in all four channels and still takes part in the
 *               sum.  CLAMP: min(max(i, 0), n - 1).  REPEAT: i mod n, non-negative.  MIRROR: m = i mod 2 n; m if m < n, otherwise
 *               2 n - 1 - m.
 *   sum         binary32.  The operand p is the f16 texel widened, its colour times its alpha unless STRAIGHT (exact).  For each tap
 *               row j ascending: H_j = 0.0f, then H_j = fmaf(wx_i, p[i][j], H_j) for i ascending.  Then V = 0.0f and V =
 *               fmaf(wy_j, H_j, V) for j ascending.  Rows before columns, as in Resample; a zero weight still multiplies.
 *   store       STRAIGHT: f16(V) per channel, round to nearest even.  Otherwise as fine, jh_composite and jh_resample store: a_inv =
 *               1.0f / max(V.a, 1e-6f); (f16(V.r a_inv + 0.0f), f16(V.g a_inv + 0.0f), f16(V.b a_inv + 0.0f), f16(V.a + 0.0f)).
 *   values      f16 subnormals are values, Inf and NaN follow IEEE, a NaN result is any NaN.  Nothing is clamped: BICUBIC can
 *               overshoot.
 * So under STRAIGHT the identity, an integer translation under ZERO and the eight flips and quarter turns are copies or permutations
 * of every finite value for every filter and edge (a -0 comes out as +0), and BILINEAR keeps a constant image constant.
 * What the rule does not do: no minification prefilter -- below about 1:2 the result aliases, jh_resample comes first for that, and
 * the limit of 64 is only there to bound the integers; no perspective (that is jh_perspective, below); no call in place.
 *
 * jh_warp_plan: P, Q, R, S, T, W of a matrix into plan.  Host only, no context.  JH_ERR_INVALID for an illegal matrix.
 * jh_warp_bounds: a rectangle {x, y, width, height} of the dst_w x dst_h image into rect such that under EDGE_ZERO every destination
 * texel outside it is transparent black: the forward images (binary64, uncontracted, (a x + c y) + e and (b x + d y) + f) of the
 * four corners of the src_w x src_h source rectangle grown by m = 0.5 NEAREST, 1 BILINEAR, 2 BICUBIC; floor(min) - 1 and ceil(max) +
 * 1, clipped to the destination; an empty result is 0, 0, 0, 0.  Host only, no context.  JH_ERR_INVALID for an illegal matrix, an
 * unknown filter or a side above 32768.
 *
 * jh_warp: the rule from the rectangle (src_x, src_y, src_width, src_height) of src_image_id into the rectangle (dst_x, dst_y,
 * dst_width, dst_height) of dst_image_id, another image; the images carry their own sizes.  Only the destination rectangle is
 * written; a dst that was never written is cleared to transparent black first and then counts as written; a source that was never
 * written reads as transparent black.  Stream-ordered on the context's stream, never waits: ONE kernel launch, plus a fill when dst
 * has to be cleared.  No scratch and no tables: the call is always capturable.  With profiling on the call is a query "warp" with
 * stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band): the rows a tap reads belong to another rank's context.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_warp: ": a null
 * desc; an unknown source or destination id; an image that is not RGBA16F; an unknown filter, edge or flag bit; an illegal matrix
 * (the message names the condition that failed); an image side above 32768; a rectangle that is not inside its image or that is
 * empty in exactly one dimension; src_image_id == dst_image_id; a band set with jh_set_band. */
typedef enum jh_warp_filter { JH_WARP_NEAREST = 0, JH_WARP_BILINEAR = 1, JH_WARP_BICUBIC = 2 } jh_warp_filter;
typedef enum jh_warp_edge { JH_WARP_EDGE_ZERO = 0, JH_WARP_EDGE_CLAMP = 1, JH_WARP_EDGE_REPEAT = 2, JH_WARP_EDGE_MIRROR = 3 } jh_warp_edge;
#define JH_WARP_STRAIGHT 1u
#define JH_WARP_MAX_SIDE 32768u
typedef struct jh_warp_desc {
    double matrix[6];                                 /* (a, b, c, d, e, f): source rectangle -> destination image */
    int filter;                                       /* jh_warp_filter */
    int edge;                                         /* jh_warp_edge */
    uint32_t flags;                                   /* bit 0: JH_WARP_STRAIGHT */
    uint32_t src_x, src_y, src_width, src_height;     /* source rectangle; width == height == 0: the whole image */
    uint32_t dst_x, dst_y, dst_width, dst_height;     /* destination rectangle, likewise */
} jh_warp_desc;
int jh_warp_plan(const double matrix[6], int64_t plan[6]);
int jh_warp_bounds(const double matrix[6], uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t rect[4]);
int jh_warp(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_warp_desc* desc);

/* ---- Convolve: feConvolveMatrix, a small non-separable convolution with arbitrary weights (DESIGN.md 5.13 "Convolve rule") ----
 * Sharpen, emboss, Sobel and Laplacian edge detection, a box or tent of the caller's choosing, any kernel up to 15 x 15 -- without the
 * image leaving the device.  The result is defined on values, and every implementation produces these bits (include/jello_convolve.h
 * states the host half, tests/convolve_ref.py restates all of it).
 *   arguments   order_x, order_y: integers in [1, JH_CONVOLVE_MAX_ORDER = 15].  target_x < order_x, target_y < order_y.
 *               weights[JH_CONVOLVE_MAX_TAPS = 225]: binary32, inline in the descriptor, row-major with stride order_x; only the first
 *               order_x order_y are read.  edge: JH_CONVOLVE_EDGE_ZERO = 0 | _CLAMP = 1 | _REPEAT = 2 | _MIRROR = 3 (jh_warp_edge's
 *               values: none, duplicate and wrap of the specification, plus mirror).  mode: JH_CONVOLVE_PREMULTIPLIED = 0 |
 *               JH_CONVOLVE_STRAIGHT = 1 | JH_CONVOLVE_PRESERVE_ALPHA = 2.  bias: binary32.  The rectangle (x, y, width, height) of
 *               dst is written; width == height == 0 means the whole image (x and y are then ignored).
 *   legal       every weight that is read and the bias are finite.
 *   weights     ARE IN THE ORDER THEY ARE APPLIED, a correlation: w[j][i] multiplies the operand at the image position (X - target_x
 *               + i, Y - target_y + j).  The 180-degree flip and the divisor of feConvolveMatrix are the host's job
 *               (jh_convolve_weights); the device never divides.
 *   operand     the f16 texel widened to binary32.  PREMULTIPLIED: colour times alpha (exact; Inf x 0 is a NaN).  STRAIGHT: the four
 *               channels as stored.  PRESERVE_ALPHA: the three colour channels as stored; the alpha channel is not convolved.
 *   edge        the IMAGE is the edge, not the rectangle (as for blur and morphology).  A tap index is resolved per axis with exactly
 *               jwarp_index(edge, i, n) of include/jello_warp.h against the image's extent n: ZERO: outside [0, n) the operand is
 *               +0.0f in all channels and still takes part in the sum; CLAMP: min(max(i, 0), n - 1); REPEAT: i mod n, non-negative;
 *               MIRROR: m = i mod 2 n; m if m < n, otherwise 2 n - 1 - m.  A source that was never written reads as transparent black.
 *   sum         per channel ONE chain in binary32: acc = +0.0f; for j ascending, for i ascending: acc = fmaf(w[j][i], p(i, j), acc).
 *               A zero weight still multiplies (0 x Inf is a NaN, as in Warp).  No per-row partial sums.
 *   bias        if bias is +-0 this step does not exist and V = acc.  Otherwise STRAIGHT: V.c = acc.c + bias for all four channels;
 *               PRESERVE_ALPHA: the same for the three colour channels; PREMULTIPLIED: V.a = acc.a + bias, then V.c = fmaf(bias, V.a,
 *               acc.c) for colour (Filter Effects' bias ALPHA with the result's alpha).  Each operation is rounded once.
 *   store       STRAIGHT: f16(V) per channel, round to nearest even.  PREMULTIPLIED: as fine, jh_composite and jh_resample store:
 *               a_inv = 1.0f / max(V.a, 1e-6f); (f16(V.r a_inv + 0.0f), f16(V.g a_inv + 0.0f), f16(V.b a_inv + 0.0f), f16(V.a +
 *               0.0f)).  PRESERVE_ALPHA: colour f16(V.c); alpha is the 16 bits of the source texel at (X, Y), copied (+0 for a
 *               never-written source).
 *   values      f16 subnormals are values, Inf and NaN follow IEEE, a NaN result is any NaN.  Nothing is clamped: jh_color_filter
 *               with clamp comes after where [0, 1] is wanted.
 * So under STRAIGHT the 1 x 1 kernel [1] copies every non-NaN value (a -0 comes out as +0: +0 + (-0)), and a kernel with a single 1
 * at (i, j) and zeros elsewhere is the integer translation by (i - target_x, j - target_y) of every finite image under ZERO.  A
 * constant image c under a kernel whose weights sum to 1 exactly stays c under CLAMP, REPEAT and MIRROR only up to the chain's
 * rounding: |V - c| <= gamma_n |c| sum |w|, gamma_n = n u / (1 - n u), n = order_x order_y, u = 2^-24, before the store's half ULP
 * -- a bound, not equality (weights whose partial sums are all exact, such as a box of 1/4, do give c).
 * What the rule does not do: no call in place; no order above 15; zero weights are not skipped; no separable fast path; no
 * kernelUnitLength.
 *
 * jh_convolve_weights: the weights of feConvolveMatrix's kernelMatrix (order_x order_y binary64, row-major) and divisor:
 * weights[j ox + i] = (float)(kernel_matrix[(oy - 1 - j) ox + (ox - 1 - i)] / d), the quotient in binary64, rounded once to binary32;
 * d = divisor if it is not 0, otherwise the sum of kernel_matrix in ascending index order in binary64, or 1.0 if that sum is 0.  Host
 * only, no context.  JH_ERR_INVALID for an order outside [1, 15], a non-finite input or a weight that does not come out finite.
 *
 * jh_convolve: the rule applied to src_image_id, written to the rectangle of dst_image_id, another image of the same size (a tile
 * of a call in place would read what another tile wrote).  Texels of dst outside the rectangle keep their bits; a dst that was never
 * written is cleared to transparent black first and then counts as written.  Stream-ordered on the context's stream, never waits:
 * ONE kernel launch, plus a fill when dst has to be cleared.  No scratch and no tables -- the weights travel in the kernel
 * arguments: the call is always capturable.  With profiling on the call is a query "convolve" with stage = -1 in
 * jh_profile_collect_tree.  Not in band mode (jh_set_band): the rows a window reads belong to another rank's context.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_convolve: ": a
 * null desc; an unknown source or destination id; an image that is not RGBA16F; images of different size; src_image_id ==
 * dst_image_id; an order outside 1..15; a target outside the order; an unknown edge or mode; a weight or a bias that is not finite;
 * a rectangle that is not inside the image or that is empty in exactly one dimension; a band set with jh_set_band.  An image without
 * texels returns JH_OK. */
typedef enum jh_convolve_edge { JH_CONVOLVE_EDGE_ZERO = 0, JH_CONVOLVE_EDGE_CLAMP = 1, JH_CONVOLVE_EDGE_REPEAT = 2, JH_CONVOLVE_EDGE_MIRROR = 3 } jh_convolve_edge;
typedef enum jh_convolve_mode { JH_CONVOLVE_PREMULTIPLIED = 0, JH_CONVOLVE_STRAIGHT = 1, JH_CONVOLVE_PRESERVE_ALPHA = 2 } jh_convolve_mode;
#define JH_CONVOLVE_MAX_ORDER 15u
#define JH_CONVOLVE_MAX_TAPS 225u
typedef struct jh_convolve_desc {
    uint32_t order_x, order_y;
    uint32_t target_x, target_y;
    int edge;                      /* jh_convolve_edge */
    int mode;                      /* jh_convolve_mode */
    float bias;
    uint32_t x, y, width, height;  /* rectangle of dst that is written; 0 x 0: the whole image */
    float weights[JH_CONVOLVE_MAX_TAPS];  /* row-major, stride order_x, in the order they are applied */
} jh_convolve_desc;
int jh_convolve_weights(uint32_t order_x, uint32_t order_y, const double* kernel_matrix, double divisor, float* weights);
int jh_convolve(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_convolve_desc* desc);

/* ---- Lighting: feDiffuseLighting and feSpecularLighting with their three light sources (DESIGN.md 5.14 "Lighting rule") ----
 * Bevels, embossed text, glossy buttons, a lit height map -- the alpha channel of src is the height, and the image never leaves the
 * device.  The result is defined on values, and every implementation produces these bits (include/jello_lighting.h states the host
 * half and the normal, tests/lighting_ref.py restates all of it).  Only the alpha channel of src is read.
 *   arguments   kind: JH_LIGHTING_DIFFUSE = 0 | JH_LIGHTING_SPECULAR = 1.  light: JH_LIGHT_DISTANT = 0 | JH_LIGHT_POINT = 1 |
 *               JH_LIGHT_SPOT = 2.  surface_scale: binary32, finite.  constant (kd or ks): binary32, finite, >= 0.
 *               specular_exponent: binary32 in [1, 128], read only under SPECULAR.  color[3]: binary32, finite, >= 0, LINEAR (the
 *               target is linear; decoding lighting-color from sRGB is the caller's job).  direction[3]: binary64, finite, TOWARDS the
 *               light, its length in binary64 finite and not 0; DISTANT only (no azimuth and no elevation: no trigonometry is in the
 *               rule).  position[3]: binary64, each finite as a binary32; POINT and SPOT.  points_at[3]: binary64, points_at - position
 *               of finite non-zero length; SPOT only.  spot_exponent: binary32 in [1, 128]; SPOT only.  cone_cos: binary64 in [-1, 1],
 *               the cosine of the limiting cone angle, -1: no cone; SPOT only.  The rectangle (x, y, width, height) of dst is written;
 *               width == height == 0 means the whole image.  Fields the kind and the light do not use are not looked at.
 *   space       coordinates are texels of the image; texel (X, Y) sits at (X + 0.5, Y + 0.5), the renderer's pixel centre.  An image
 *               extent above 2^23 is refused, so that (float)X + 0.5f is exact.
 *   plan        jh_lighting_plan (a jh_light_plan), on the host, the only place binary64 appears: s[span - 1][wsum - 2] = (float)(-(double)surface_scale
 *               * 2.0 / (double)(span * wsum)) for span in {1, 2}, wsum in {2, 3, 4};  ldir = direction / |direction|, |d| = sqrt(x x +
 *               y y + z z) in binary64 left to right, each quotient rounded once to binary32;  p = (float)position;  sdir = (points_at -
 *               position) normalised the same way;  cone = (float)cone_cos.  What the light does not use is +0.
 *   normal      A(i, j): the f16 alpha of src at column i, row j, widened to binary32 (a never-written src: +0).  x_lo = max(X - 1, 0),
 *               x_hi = min(X + 1, W - 1), rows likewise -- the IMAGE is the edge, not the rectangle.  span_x = x_hi - x_lo; wsum_y = the
 *               sum of the weights (1, 2, 1) over those of the rows Y - 1, Y, Y + 1 that exist.  c(col) = the sum over the existing rows,
 *               ASCENDING, of w_j A(col, j), in binary32, the adds left to right (2 A is exact).  gx = c(x_hi) - c(x_lo); Nx =
 *               s(span_x, wsum_y) gx.  Ny likewise with row sums r(row) over the existing columns ascending, gy = r(y_hi) - r(y_lo), Ny =
 *               s(span_y, wsum_x) gy.  An axis with span 0 (an image one texel wide or high) gives +0 for its component.  These are the
 *               specification's nine cases (interior, four edges, four corners: factors 1/4, 1/3, 1/2 and 2/3; DESIGN.md 5.14 lists
 *               them).  nlen = sqrtf(fmaf(Nx, Nx, fmaf(Ny, Ny, 1.0f))); the normal is (Nx, Ny, 1) / nlen, never normalised by itself.
 *   light       DISTANT: l = ldir, not renormalised.  POINT and SPOT: Z = surface_scale A(X, Y); v = (p.x - ((float)X + 0.5f), p.y -
 *               ((float)Y + 0.5f), p.z - Z); len = sqrtf(fmaf(v.z, v.z, fmaf(v.y, v.y, v.x v.x))); l = v / len, three IEEE divisions.
 *   colour      DISTANT and POINT: C = color.  SPOT: m = -fmaf(l.z, sdir.z, fmaf(l.y, sdir.y, l.x sdir.x)); if not (m > 0 and m >= cone)
 *               C = +0 in all channels (a NaN lands here; the cone's edge is hard); otherwise C.c = color.c Pw(min(m, 1), spot_exponent).
 *   power       Pw(t, 1.0f) = t.  Otherwise a table of JH_LIGHTING_TABLE_ENTRIES = 4097 binary32, T[i] = (float)pow((double)i / 4096.0,
 *               (double)e) -- libm in binary64, rounded once;  u = t 4096.0f (exact); i = min((int)u, 4095); f = u - (float)i (exact);
 *               Pw = fmaf(f, T[i + 1] - T[i], T[i]), the difference one binary32 subtraction.  |Pw - t^e| <= e (e - 1) / (8 4096^2) for e
 *               >= 2, and <= 4096^-e for 1 < e < 2 (the first segment), before the rounding: DESIGN.md 5.14.
 *   DIFFUSE     t = fmax(fmaf(Nx, l.x, fmaf(Ny, l.y, l.z)) / nlen, 0.0f) (maxNum: a NaN gives 0); k = constant t; V.c = fmin(k C.c,
 *               1.0f); the texel is (f16(V.r), f16(V.g), f16(V.b), 0x3c00).
 *   SPECULAR    h = (l.x, l.y, l.z + 1.0f); hlen = sqrtf(fmaf(h.z, h.z, fmaf(h.y, h.y, h.x h.x))); q = fmaf(Nx, h.x, fmaf(Ny, h.y, h.z)) /
 *               (nlen hlen); t = Pw(fmin(fmax(q, 0.0f), 1.0f), specular_exponent); k = constant t; V.c = fmin(k C.c, 1.0f); a = max(V.r,
 *               V.g, V.b); the store is fine's un-premultiplying one, as jh_convolve PREMULTIPLIED: a_inv = 1.0f / max(a, 1e-6f);
 *               (f16(V.c a_inv + 0.0f), f16(a + 0.0f)).
 *   values      no contraction beyond the fmaf written above; IEEE divide and sqrt; every operation rounded once; min and max are
 *               minNum and maxNum; f16 subnormals are values; an Inf or NaN alpha follows these operations and nothing else; a NaN
 *               result is any NaN.
 * So a constant finite alpha gives N = (0, 0, 1) and DIFFUSE DISTANT is min(kd ldir.z color, 1) everywhere; a light below the
 * surface gives black; a SPECULAR texel's alpha is the maximum of its premultiplied colour.
 * What the rule does not do: no kernelUnitLength; no antialiased cone edge; no light in user units (a caller with a transform maps the
 * light itself); no call in place; no second resident table set.
 *
 * jh_lighting_plan: the plan of desc.  jh_lighting_tables: the tables desc needs -- *which = JH_LIGHTING_TABLE_SPEC (SPECULAR with
 * specular_exponent != 1) | JH_LIGHTING_TABLE_SPOT (SPOT with spot_exponent != 1); each that is needed is written where its pointer is
 * not NULL.  Both host only, no context; JH_ERR_INVALID for a null or illegal desc (the rectangle is not looked at).
 *
 * jh_lighting: the rule applied to src_image_id, written to the rectangle of dst_image_id, another image of the same size (a tile of
 * a call in place would read alpha that another tile overwrote).  Texels of dst outside the rectangle keep their bits; a dst that was
 * never written is cleared to transparent black first and then counts as written.  Stream-ordered, never waits: ONE kernel launch,
 * plus a fill when dst has to be cleared.  The context keeps the tables of ONE key -- the bit patterns of the two exponents where
 * their table is needed, 0 otherwise -- in a scratch slot of their own, by the contract of jh_resample and jh_color_filter: repeating
 * the key uploads nothing and is capturable; another key uploads its tables, bumps the generation and makes earlier graphs stale; a
 * capture whose tables are not resident is refused (JH_ERR_OOM, "run this lighting once eagerly first"); a call that needs no table
 * (DIFFUSE with DISTANT or POINT, any call whose exponents in use are 1) is always capturable and does not touch the slot;
 * jh_scratch_trim forgets the key.  With profiling on the call is a query "lighting" with stage = -1 in jh_profile_collect_tree.  Not
 * in band mode (jh_set_band).  JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that
 * starts "jh_lighting: ": a null desc; an unknown source or destination id; an image that is not RGBA16F; images of different size;
 * src_image_id == dst_image_id; an extent above 2^23; an unknown kind or light; an illegal field of the list above; a rectangle that
 * is not inside the image or that is empty in exactly one dimension; a band set with jh_set_band.  An image without texels returns
 * JH_OK. */
typedef enum jh_lighting_kind { JH_LIGHTING_DIFFUSE = 0, JH_LIGHTING_SPECULAR = 1 } jh_lighting_kind;
typedef enum jh_light_source { JH_LIGHT_DISTANT = 0, JH_LIGHT_POINT = 1, JH_LIGHT_SPOT = 2 } jh_light_source;
#define JH_LIGHTING_TABLE_ENTRIES 4097u
#define JH_LIGHTING_TABLE_SPEC 1u
#define JH_LIGHTING_TABLE_SPOT 2u
#define JH_LIGHTING_MAX_EXTENT 8388608u /* 2^23 */
typedef struct jh_lighting_desc {
    int kind;                      /* jh_lighting_kind */
    int light;                     /* jh_light_source */
    float surface_scale;
    float constant;                /* kd or ks */
    float specular_exponent;
    float spot_exponent;
    float color[3];                /* linear */
    uint32_t x, y, width, height;  /* rectangle of dst that is written; 0 x 0: the whole image */
    double direction[3];           /* towards the light */
    double position[3];
    double points_at[3];
    double cone_cos;
} jh_lighting_desc;
typedef struct jh_light_plan {
    float s[2][3];  /* [span - 1][wsum - 2] */
    float ldir[3];
    float p[3];
    float sdir[3];
    float cone;
} jh_light_plan;
int jh_lighting_plan(const jh_lighting_desc* desc, jh_light_plan* plan);
int jh_lighting_tables(const jh_lighting_desc* desc, float* spec_table /* 4097 or NULL */, float* spot_table /* 4097 or NULL */, uint32_t* which);
int jh_lighting(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_lighting_desc* desc);

/* ---- Turbulence: feTurbulence, Perlin turbulence or fractal noise GENERATED into an image (DESIGN.md 5.15 "Turbulence rule") ----
 * Grain, clouds, marble, the height map jh_lighting reads, a mask for jh_composite -- made where the other calls run, nothing is
 * uploaded but 8.4 KB of tables per seed.  The algorithm is the reference code of Filter Effects Level 1 (the stitch comparison BEFORE
 * the mask with 255).  The result is defined on values, and every implementation produces these bits (include/jello_turbulence.h states
 * the host half and the device half's cases, tests/turbulence_ref.py restates all of it).  Binary64 appears in the plan and the tables
 * only.  The image holds straight colour and so does the primitive's result: the four channels are stored as they come.
 *   arguments   kind: JH_TURBULENCE_FRACTAL_NOISE = 0 | JH_TURBULENCE_TURBULENCE = 1.  base_frequency[2]: binary64, finite, >= 0, in
 *               cells per texel.  octaves: 0 .. JH_TURBULENCE_MAX_OCTAVES = 16.  seed: int32.  stitch: 0 or 1.  tile[4]: binary64 x, y,
 *               w, h, finite, w and h > 0; read only under stitch.  origin[2]: binary64, finite: the coordinate of the image's corner,
 *               so that a caller can continue one noise field across images.  The rectangle (x, y, width, height) of dst is written;
 *               width == height == 0 means the whole image.
 *   space       the centre of texel (X, Y) of the IMAGE is at (origin.x + X + 0.5, origin.y + Y + 0.5).
 *   seed        the specification's setup_seed, in integers, m = 2^31 - 1: s <= 0 becomes -(s mod (m - 1)) + 1 (C's remainder), s >
 *               m - 1 becomes m - 1.  That value is the KEY of the tables.
 *   tables      the specification's init with the Park-Miller generator (a = 16807, m = 2^31 - 1, Schrage's q = 127773, r = 2836;
 *               from seed 1 the 10 000th number is 1043618065), the draws in its order: the gradients first, k = 0 .. 3 outermost, i =
 *               0 .. 255, x then y, each ((r mod 512) - 256) / 256, which is exact; s = sqrt(x x + y y) in binary64 left to right;
 *               G[k][i] = ((float)(x / s), (float)(y / s)), each quotient in binary64 rounded once.  A gradient whose components are
 *               both 0 is 0 / 0 in the specification's code; here it stays (+0, +0).  Then the shuffle of P[i] = i: for i = 255 down to
 *               1, swap P[i] and P[r mod 256].  The specification's duplicated upper halves are not stored: its P[i + by] with i + by up
 *               to 510 is P[(i + by) & 255] by construction, which is what the rule reads (tools/turbulence_check.cpp compares them).
 *   plan        jh_turbulence_plan (a jh_turb_plan), on the host.  Per axis f = base_frequency; under stitch and f != 0 the
 *               specification's lo / hi rule in binary64: t = tile_w f, lo = floor(t) / tile_w, hi = ceil(t) / tile_w, f = lo if lo !=
 *               0 and f / lo < hi / f, else hi.  Under stitch width = (int)(tile_w f + 0.5) and wrap = floor(tile_x f) + width, with
 *               the adjusted f (the specification's + 4096 is dropped from both sides of its comparison); otherwise both are 0.
 *               Positions are int64 in units of 2^-32 cell: step = nearbyint(f 2^32), start = nearbyint(((origin + 0.5) f) 2^32) --
 *               the sum, the product and the (exact) scaling one binary64 operation each, ties to even --, pos(X) = start + X step.
 *   legal       with L = (2^62 - 1) >> max(octaves - 1, 0): f 2^32 and |(origin + 0.5) f 2^32| below 2^62; |start| <= L; the image
 *               extent at most max_extent = the largest W with start + (W - 1) step <= L -- so every position of the IMAGE shifted
 *               left by octaves - 1 fits an int64 with a bit to spare --; under stitch tile_w f + 0.5 and |floor(tile_x f)| below 2^31
 *               and |wrap|, width <= (2^31 - 1) >> max(octaves - 1, 0).  Anything else is refused with a message.
 *   octave      for k = 0 .. octaves - 1, per axis: p = pos << k; cell i = p >> 32 (arithmetic: negative coordinates floor); r0 =
 *               (float)((uint32)p >> 8) 2^-24 (exact), r1 = r0 - 1.0f (exact).  Under stitch wrap_k = wrap << k, width_k = width << k,
 *               and each of i and i + 1 that is >= wrap_k has width_k subtracted; then the mask with 255: bx0, bx1, by0, by1.
 *   lattice     b00 = P[(P[bx0] + by0) & 255], b10 = P[(P[bx1] + by0) & 255], b01 = P[(P[bx0] + by1) & 255], b11 = P[(P[bx1] + by1)
 *               & 255].
 *   noise       s(t) = (t t) fmaf(-2.0f, t, 3.0f); sx = s(rx0), sy = s(ry0).  For channel c (r, g, b, a = 0 .. 3) and corner b.. with
 *               g = G[c][b..] and (rx, ry) the offset to that corner -- (rx0, ry0), (rx1, ry0), (rx0, ry1), (rx1, ry1) --: u.. =
 *               fmaf(ry, g.y, rx g.x).  lerp(t, a, b) = fmaf(t, b - a, a); n = lerp(sy, lerp(sx, u00, u10), lerp(sx, u01, u11)).
 *               sum = fmaf(n, 2^-k, sum) under FRACTAL_NOISE, fmaf(|n|, 2^-k, sum) under TURBULENCE, from +0.
 *   result      v = fmaf(sum, 0.5f, 0.5f) under FRACTAL_NOISE, v = sum under TURBULENCE; fmin(fmax(v, 0.0f), 1.0f); the texel is
 *               the four values rounded once to f16.  No contraction beyond the fmaf written here; every operation rounded once.
 * So with 0 octaves FRACTAL_NOISE gives 0.5 in all four channels and TURBULENCE transparent black, and the noise is exactly 0 where
 * the position is a lattice point in every octave.  The stored texel is within 2^-12 (half an f16 ULP below 1) + 10.5 (K (W + 2) 2^-33 +
 * 2^-23) + (40 + 2 K) 2^-24 of the specification's binary64 code, K octaves on an image extent W, positions up to 2^20 cells: DESIGN.md
 * 5.15 derives it.
 * What the rule does not do: no colour-space conversion (the target is linear, as color-interpolation-filters defaults); no user-unit
 * scale (the caller scales the frequency); stitched tiles repeat only to within the position grid -- the step is rounded to 2^-32
 * cell, so after tile_w texels the position is off by at most tile_w 2^-33 cell per octave step, which is not bit-periodic (DESIGN.md
 * 5.15 has the bound in f16 ULP) --; no second resident table set; no float seed.
 *
 * jh_turbulence_plan: the plan of desc (the rectangle is not looked at; the image extent is checked against max_extent by
 * jh_turbulence).  jh_turbulence_tables: selector[256] = P and gradients[2048] = G[4][256][2] of desc's seed (either may be NULL).
 * Both host only, no context; JH_ERR_INVALID for a null or illegal desc.
 *
 * jh_turbulence: the rule, written to the rectangle of dst_image_id.  Texels of dst outside the rectangle keep their bits; a dst that
 * was never written is cleared to transparent black first and then counts as written.  Stream-ordered, never waits: ONE kernel
 * launch, plus a fill when dst has to be cleared.  The context keeps the tables of ONE key (the seed after setup_seed) in a scratch
 * slot of their own, by the contract of jh_lighting: repeating the key uploads nothing and is capturable; another key uploads its
 * tables, bumps the generation and makes earlier graphs stale; a capture whose tables are not resident is refused (JH_ERR_OOM, "run
 * this turbulence once eagerly first"); jh_scratch_trim forgets the key.  With profiling on the call is a query "turbulence" with
 * stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band).  JH_ERR_INVALID, with nothing enqueued, no memory touched and
 * nothing flushed, each with a message that starts "jh_turbulence: ": a null desc; an unknown destination id; an image that is not
 * RGBA16F; an unknown kind; more than 16 octaves; a stitch that is neither 0 nor 1; an illegal field of the list above; an image
 * beyond max_extent; a rectangle that is not inside the image or that is empty in exactly one dimension; a band set with jh_set_band.
 * An image without texels returns JH_OK. */
typedef enum jh_turbulence_kind { JH_TURBULENCE_FRACTAL_NOISE = 0, JH_TURBULENCE_TURBULENCE = 1 } jh_turbulence_kind;
#define JH_TURBULENCE_MAX_OCTAVES 16u
typedef struct jh_turbulence_desc {
    int kind;                      /* jh_turbulence_kind */
    uint32_t octaves;
    int32_t seed;
    int stitch;
    uint32_t x, y, width, height;  /* rectangle of dst that is written; 0 x 0: the whole image */
    double base_frequency[2];      /* cells per texel */
    double tile[4];                /* x, y, w, h; under stitch */
    double origin[2];              /* the coordinate of the image's corner */
} jh_turbulence_desc;
typedef struct jh_turb_plan {
    double frequency[2];     /* after the stitch adjustment */
    int64_t step[2];         /* 2^-32 cell per texel */
    int64_t start[2];        /* the position of texel 0 */
    int32_t wrap[2];         /* under stitch, else 0 */
    int32_t width[2];
    uint32_t max_extent[2];  /* the largest legal image extent */
    uint32_t key;            /* the seed after setup_seed */
    uint32_t stitched;
} jh_turb_plan;
int jh_turbulence_plan(const jh_turbulence_desc* desc, jh_turb_plan* plan);
int jh_turbulence_tables(const jh_turbulence_desc* desc, uint8_t* selector /* 256 or NULL */, float* gradients /* 2048 or NULL */);
int jh_turbulence(jh_ctx* ctx, uint64_t dst_image_id, const jh_turbulence_desc* desc);

/* ---- Displace: feDisplacementMap, a warp whose positions a second image moves texel by texel (DESIGN.md 5.17 "Displacement rule") ----
 * Heat haze, ripples, a noise-roughened edge, frosted glass -- without the frame or the noise leaving the device.  The result is
 * defined on values, and every implementation produces these bits (include/jello_displace.h states the host half,
 * tests/displace_ref.py restates all of it).
 *   arguments   matrix[6], filter, edge, flags (bit 0: JH_DISPLACE_STRAIGHT) and the source and destination rectangles: exactly
 *               jh_warp_desc's, with the same meaning and the same legality -- the matrix takes continuous coordinates of the SOURCE
 *               RECTANGLE to continuous coordinates of the DESTINATION IMAGE, and the identity is what feDisplacementMap needs.
 *               scale_x, scale_y: binary32, finite, in texels of the source rectangle per unit of map value.  x_channel, y_channel:
 *               JH_DISPLACE_R = 0 | _G = 1 | _B = 2 | _A = 3, which channel of the map moves which axis (they may be the same).
 *   plan        jh_warp_plan's six integers P, Q, R, S, T, W, unchanged.
 *   map         an RGBA16F image of the destination IMAGE's size.  For destination texel (X, Y) of the image the map value m is the
 *               stored f16 of the chosen channel of the map's texel (X, Y), widened to binary32.  Stored texels are un-premultiplied,
 *               which is what the specification asks of in2; JH_DISPLACE_STRAIGHT does not change how the map is read.  A map that
 *               was never written reads 0 in every channel.  No colour-space conversion of the map.
 *   offset      per axis: t = m - 0.5f (exact for every finite f16: at most 24 significant bits).  d = scale t, ONE binary32
 *               product.  A NaN d (a NaN m, 0 x Inf) counts as +0; otherwise d is clamped to [-2^22, 2^22].  D = (int64) rint(d 2^32),
 *               ties to even; the scaling and the conversion are exact after the clamp.
 *   position    U = P (2 X + 1) + Q (2 Y + 1) + R + Dx, V = S (2 X + 1) + T (2 Y + 1) + W + Dy, int64, |U| < 2^56: the source position
 *               in units of 2^-32 texel.  The displacement is in texels of the source rectangle and is added AFTER the affine map.
 *               Under a translation (all the specification needs) that equals displacing in destination space; under a general
 *               matrix it does not -- the rule does not apply the matrix's linear part to the displacement.
 *   taps, edge, sum, store, values: jh_warp's, word for word, at (U, V): NEAREST is a floor, the fraction's low 16 bits are dropped,
 *               BICUBIC's weights are jh_warp's; a tap index is resolved against the source RECTANGLE's extent; rows then columns
 *               with single fmaf's; the operand is premultiplied unless JH_DISPLACE_STRAIGHT; the un-premultiplying store.
 * So with scale = (0, 0), or with a map that is 0.5 in both chosen channels, the result is jh_warp's bit for bit; a constant map with
 * scale t an integer is the integer translation by it; a call written in four quadrant rectangles equals the whole-image call.
 *
 * jh_displace_offset: D for one scale and one f16 bit pattern into *out.  Host only, no context; JH_ERR_INVALID for a null out (a
 * non-finite scale is computed, by the rule's words; jh_displace refuses it).
 *
 * jh_displace: the rule from the rectangle (src_x, ...) of src_image_id into the rectangle (dst_x, ...) of dst_image_id, another
 * image, moved by map_image_id.  THE MAP MAY BE THE DESTINATION: a texel's map value is read before that texel is written and by
 * nothing else, so noise generated into an image (jh_turbulence) and then displaced over in place needs no third image.  The map may
 * be the source too.  Only the destination rectangle is written; a dst that was never written is cleared to transparent black first
 * (and, being the map as well, then reads 0) and then counts as written; a source that was never written reads as transparent black.
 * Stream-ordered on the context's stream, never waits: ONE kernel launch, plus a fill when dst has to be cleared.  No scratch and
 * no tables: the call is always capturable.  With profiling on the call is a query "displace" with stage = -1 in
 * jh_profile_collect_tree.  Not in band mode (jh_set_band): the rows a tap reads belong to another rank's context.  JH_ERR_INVALID,
 * with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_displace: ": everything jh_warp
 * refuses (a null desc; an unknown source or destination id; an image that is not RGBA16F; an unknown filter, edge or flag bit; an
 * illegal matrix; an image side above 32768; a rectangle that is not inside its image or that is empty in exactly one dimension;
 * src_image_id == dst_image_id; a band); an unknown map id; a map that is not RGBA16F; a map whose size is not dst's; a channel
 * outside 0..3; a scale that is not finite. */
typedef enum jh_displace_channel { JH_DISPLACE_R = 0, JH_DISPLACE_G = 1, JH_DISPLACE_B = 2, JH_DISPLACE_A = 3 } jh_displace_channel;
#define JH_DISPLACE_STRAIGHT 1u
typedef struct jh_displace_desc {
    double matrix[6];                                 /* (a, b, c, d, e, f): source rectangle -> destination image */
    int filter;                                       /* jh_warp_filter */
    int edge;                                         /* jh_warp_edge */
    uint32_t flags;                                   /* bit 0: JH_DISPLACE_STRAIGHT */
    uint32_t src_x, src_y, src_width, src_height;     /* source rectangle; width == height == 0: the whole image */
    uint32_t dst_x, dst_y, dst_width, dst_height;     /* destination rectangle, likewise */
    float scale_x, scale_y;                           /* texels of the source rectangle per unit of map value */
    int x_channel, y_channel;                         /* jh_displace_channel */
} jh_displace_desc;
int jh_displace_offset(float scale, uint16_t f16_bits, int64_t* out);
int jh_displace(jh_ctx* ctx, uint64_t src_image_id, uint64_t map_image_id, uint64_t dst_image_id, const jh_displace_desc* desc);

/* ---- Shadow: the Gaussian blur of a rounded rectangle, GENERATED into an image or laid over it (DESIGN.md 5.18 "Shadow rule") ----
 * The shadow under a card, a button, a window: the blur of this shape has a form that needs no source image, no intermediate and no
 * blur pass, and its cost does not depend on sigma.  The result is defined on values, and every implementation produces these bits
 * (include/jello_shadow.h states the host half and the device half's functions, tests/shadow_ref.py restates all of it).  Binary64
 * appears in the plan and the bounds only.
 *   arguments   the rectangle (x, y, width, height) of dst that is written (all zero: the whole image).  matrix[6]: binary64, (a, b,
 *               c, d, e, f), x' = a x + c y + e, y' = b x + d y + f, from SHAPE space to continuous coordinates of the destination
 *               IMAGE (texel (i, j) centred at (i + 0.5, j + 0.5)); legal as jh_warp's is.  box[4]: binary32 x0, y0, x1, y1 in shape
 *               space.  radius, sigma: binary32, shape units.  color[4]: binary32, premultiplied, linear; any value.  flags:
 *               JH_SHADOW_OVER = 1 | JH_SHADOW_INVERT = 2.
 *   legal       the box finite with x1 >= x0 and y1 >= y0 (empty in a dimension is legal: S = 0) and every coordinate within
 *               [-2^22, 2^22]; radius finite and >= 0; sigma finite and in [0, 2^16]; no other flag bit; image extents at most 2^23.
 *   plan        jh_shadow_plan (a jh_shad_plan), on the host, binary64, every operation rounded once: m = jh_warp_plan's six integers of the matrix;
 *               centre = (x0 + x1) / 2, a = (x1 - x0) / 2, likewise y and b; r = min(radius, a, b) (CSS's clamp); sigma' = max(sigma,
 *               2^-8) (below it: the point-sampled shape); C = rint(centre 2^32); then, each rounded once to binary32: a, b, r, core =
 *               a - r, straight = b - r, sigma', inv_s = 1 / (sigma' sqrt 2), window = K sigma' with K = 4.  N = 4 where r / sigma' <=
 *               0.5, 8 where <= 1.5, else 16.
 *   position    for destination texel (X, Y) of the image: U = m0 (2 X + 1) + m1 (2 Y + 1) + m2 - Cx, V = m3 (2 X + 1) + m4 (2 Y + 1) +
 *               m5 - Cy, exact in int64 (below 2^63: |m0| <= 2^37, 2 X + 1 < 2^24), units of 2^-32.  x = (float)(int32)(U >> 32) +
 *               (float)((uint32)U >> 8) 2^-24: the whole part converted (exact below 2^24), the fraction's low 8 bits dropped, the sum
 *               rounded once; y of V.  The blur lives in shape space: a rotated box has a rotated shadow, and under a non-uniform
 *               scale the blur is anisotropic on the device.
 *   G(z)        the erf approximant, binary32: t = minNum(|z|, 4); u = t (a1 + t (a2 + t (a3 + t (a4 + t (a5 + t a6))))) by five fmaf
 *               from the inside and one product, (a1 .. a6) = (0.0705230784, 0.0422820123, 0.0092705272, 0.0001520143, 0.0002765672,
 *               0.0000430638) rounded to binary32; four times s = s (2 + s), from s = u; e = 1 - 1 / (1 + s), IEEE division; G =
 *               copysign(e, z).  No table.  Monotone in binary32 and exactly 1 from |z| = 4 on; Phi(t) = (1 + G(t / sqrt 2)) / 2 within
 *               2^-20 (measured 2.1e-7).
 *   band        B(p, w) = G((p + w) inv_s) - G((p - w) inv_s), each sum, difference and product rounded once.
 *   coverage    acc = B(y, straight) B(x, a).  With r > 0 the cap above, q = y - straight, then the cap below, q = -y - straight, add
 *               to acc: lo = maxNum(q - window, 0), hi = minNum(q + window, r); nothing unless hi > lo; t0 = 1 - sqrt(1 - lo / r), t1 =
 *               1 - sqrt(1 - hi / r), dt = (t1 - t0) (1 / N); m_0 = lo, m_N = hi and for 0 < i < N: t = fmaf(i, dt, t0), m_i =
 *               minNum(maxNum((r t) (2 - t), m_(i-1)), hi); for i = 1 .. N: dG = G((m_i - q) inv_s) - G((m_(i-1) - q) inv_s), mm = 0.5
 *               (m_(i-1) + m_i), w = core + sqrt((r - mm) (r + mm)), acc = fmaf(dG, B(x, w), acc).  S = minNum(0.25 acc, 1).
 *   store       S' = S, or 1 - S under JH_SHADOW_INVERT.  p = color S', one product per channel.  The texel is p by the store rule
 *               (a_inv = 1 / maxNum(p.a, 1e-6), f16(p.rgb a_inv + 0.0f), f16(p.a + 0.0f)).  Under JH_SHADOW_OVER that texel is the
 *               SOURCE of jh_composite's rule, Normal + SrcOver, opacity 1, no tint, onto the texel dst holds (never written:
 *               transparent black), word for word: so OVER equals the call without OVER into a second image followed by jh_composite,
 *               bit for bit.
 * So with r = 0 the coverage is the product of two bands, exact up to G; a box empty in a dimension gives transparent black (or
 * color under INVERT); the result is symmetric under the box's two reflections wherever the positions are.
 *
 * jh_shadow_plan: the plan of desc (the rectangle and the flags' meaning are not looked at).  jh_shadow_bounds: rect[4] = {x, y, width,
 * height} of a dst_w x dst_h destination outside which S is below 2^-12 -- the box grown by 3.625 sigma' on every side, its corners
 * through the matrix in binary64, floor(min) - 1 and ceil(max) + 1, clipped to the image; all zero when nothing is left or the box is
 * empty in a dimension.  It is how a caller restricts the call to the shadow; under INVERT it bounds S all the same, not 1 - S.  Both
 * are host only, no context; JH_ERR_INVALID for a null argument or a descriptor the rule refuses, the outputs then untouched.
 *
 * jh_shadow: the rule, written to the rectangle of dst_image_id.  Texels of dst outside the rectangle keep their bits; a dst that was
 * never written is cleared to transparent black first and then counts as written.  Stream-ordered on the context's stream, never
 * waits: ONE kernel launch, plus a fill when dst has to be cleared.  No scratch, no tables, no resident key: always capturable.  With
 * profiling on the call is a query "shadow" with stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band).
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_shadow: ": a null
 * desc; an unknown destination id; an image that is not RGBA16F; an image extent above 2^23; what the list under `legal` refuses; an
 * illegal matrix; a rectangle that is not inside the image or that is empty in exactly one dimension; a band. */
#define JH_SHADOW_OVER 1u
#define JH_SHADOW_INVERT 2u
typedef struct jh_shadow_desc {
    double matrix[6];               /* (a, b, c, d, e, f): shape space -> destination image */
    uint32_t x, y, width, height;   /* the rectangle of dst that is written; width == height == 0: the whole image */
    uint32_t flags;                 /* JH_SHADOW_OVER | JH_SHADOW_INVERT */
    float radius, sigma;            /* shape units */
    float box[4];                   /* x0, y0, x1, y1 in shape space */
    float color[4];                 /* premultiplied, linear */
} jh_shadow_desc;
typedef struct jh_shad_plan {
    int64_t m[6];        /* jh_warp_plan's P, Q, R, S, T, W */
    int64_t centre[2];   /* the box's centre, 2^-32 shape units */
    float a, b, radius;  /* the half sizes and the clamped radius */
    float core, straight; /* a - r, b - r */
    float sigma, inv_s, window; /* sigma', 1 / (sigma' sqrt 2), K sigma' */
    uint32_t n, k;       /* N and K */
} jh_shad_plan;
int jh_shadow_plan(const jh_shadow_desc* desc, jh_shad_plan* plan);
int jh_shadow_bounds(const jh_shadow_desc* desc, uint32_t dst_w, uint32_t dst_h, uint32_t* rect /* 4 */);
int jh_shadow(jh_ctx* ctx, uint64_t dst_image_id, const jh_shadow_desc* desc);

/* ---- Perspective: a projective transform of a rectangle of one RGBA16F image into a rectangle of another ----
 * A CSS perspective() / rotateX / rotateY / matrix3d card flip, a keystone correction, a layer mapped onto an arbitrary quad -- what
 * Skia, Core Animation and every browser compositor do with one 3 x 3 matrix -- without the image leaving the device.  The result is
 * defined on values, and every implementation produces these bits (include/jello_perspective.h states the plan and the position,
 * tests/perspective_ref.py restates all of it).
 *   arguments   matrix[9], binary64, column-major so that it extends jh_warp's order: (a, b, p, c, d, q, e, f, s),
 *               x' w = a x + c y + e,  y' w = b x + d y + f,  w = p x + q y + s.  It maps continuous coordinates of the SOURCE
 *               RECTANGLE (origin its top-left corner, texel (i, j) centred at (i + 0.5, j + 0.5)) to continuous coordinates of the
 *               DESTINATION IMAGE.  With p = q = 0, s = 1 it is jh_warp's matrix.  filter, edge, flags (bit 0:
 *               JH_PERSPECTIVE_STRAIGHT) and the rectangles: jh_warp_desc's, with the same meaning.
 *   plan        host only, binary64, nothing contracted, each product, difference and quotient rounded once.  The adjugate is nine
 *               two-product differences in this order:
 *                 ( d s - f q,  e q - c s,  c f - e d )
 *                 ( f p - b s,  a s - e p,  e b - a f )
 *                 ( b q - d p,  c p - a q,  a d - c b )
 *               det = ((a adj00) + (c adj10)) + (e adj20).  G = adj scaled by 2^-k, where 2^(k-1) < max |adj_ij| <= 2^k: an exact
 *               ldexp, not a division, so a matrix whose inverse is dyadic stays exact.  G is negated when det < 0: every
 *               |G_ij| <= 1, and den > 0 <=> w > 0 (in front of the viewer).
 *   legal       nine finite entries; nine finite adjugate entries; det finite and not 0; both images at most 32768 on a side.
 *   position    device, binary64, per destination texel (X, Y) of the image: x' = X + 0.5, y' = Y + 0.5 (exact);
 *               n_u = ((G0 x') + (G1 y')) + G2, likewise n_v with G3..5 and den with G6..8; q = 1.0 / den (IEEE); u = n_u q,
 *               v = n_v q.  The texel is VOID when !(den > 0) or when u or v is a NaN: it stores four +0.0 whatever the edge mode.
 *               Otherwise u is clamped to [-2^22, 2^22] and U = (int64) rint(u 2^32), half to even; V likewise: the source
 *               position in units of 2^-32 texel.
 *   taps, edge, sum, store, values: jh_warp's, word for word, at (U, V).
 * So under an affine matrix whose inverse is dyadic (the identity, integer and half-texel translations, the flips and quarter turns,
 * a scale by a power of two) the result is jh_warp's bit for bit, and a call written in four quadrant rectangles equals the
 * whole-image call.
 * What the rule does not do: no minification prefilter -- toward the horizon the result aliases, and jh_resample first is the answer
 * today; no call in place; under REPEAT / MIRROR a clamped position reads whatever the index rule gives there.
 *
 * jh_perspective_plan: the nine doubles of G into plan.  Host only, no context.  JH_ERR_INVALID for an illegal matrix.
 * jh_perspective_bounds: a rectangle {x, y, width, height} of the dst_w x dst_h image into rect such that under EDGE_ZERO every
 * destination texel outside it is transparent black: the forward images (binary64, uncontracted: xw = ((a x) + (c y)) + e,
 * yw = ((b x) + (d y)) + f, w = ((p x) + (q y)) + s, then xw / w and yw / w) of the four corners of the src_w x src_h source
 * rectangle grown by 0.5 NEAREST, 1 BILINEAR, 2 BICUBIC.  If a corner has w <= 0 the image of the rectangle is unbounded and the
 * answer is the whole destination; otherwise floor(min) - 1 and ceil(max) + 1, clipped to the destination; an empty result is
 * 0, 0, 0, 0.  Host only, no context.  JH_ERR_INVALID for an illegal matrix, an unknown filter or a side above 32768.
 *
 * jh_perspective: the rule from the rectangle (src_x, ...) of src_image_id into the rectangle (dst_x, ...) of dst_image_id, another
 * image; the images carry their own sizes.  Only the destination rectangle is written; a dst that was never written is cleared to
 * transparent black first and then counts as written; a source that was never written reads as transparent black.  Stream-ordered
 * on the context's stream, never waits: ONE kernel launch, plus a fill when dst has to be cleared.  No scratch and no tables: the
 * call is always capturable.  With profiling on the call is a query "perspective" with stage = -1 in jh_profile_collect_tree.  Not
 * in band mode (jh_set_band): the rows a tap reads belong to another rank's context.  JH_ERR_INVALID, with nothing enqueued, no
 * memory touched and nothing flushed, each with a message that starts "jh_perspective: ": a null desc; an unknown source or
 * destination id; an image that is not RGBA16F; an unknown filter, edge or flag bit; an illegal matrix (the message names the
 * condition that failed); an image side above 32768; a rectangle that is not inside its image or that is empty in exactly one
 * dimension; src_image_id == dst_image_id; a band set with jh_set_band. */
#define JH_PERSPECTIVE_STRAIGHT 1u
typedef struct jh_perspective_desc {
    double matrix[9];                                 /* (a, b, p, c, d, q, e, f, s): source rectangle -> destination image */
    int filter;                                       /* jh_warp_filter */
    int edge;                                         /* jh_warp_edge */
    uint32_t flags;                                   /* bit 0: JH_PERSPECTIVE_STRAIGHT */
    uint32_t src_x, src_y, src_width, src_height;     /* source rectangle; width == height == 0: the whole image */
    uint32_t dst_x, dst_y, dst_width, dst_height;     /* destination rectangle, likewise */
} jh_perspective_desc;
int jh_perspective_plan(const double matrix[9], double plan[9]);
int jh_perspective_bounds(const double matrix[9], uint32_t src_w, uint32_t src_h, int filter, uint32_t dst_w, uint32_t dst_h, uint32_t rect[4]);
int jh_perspective(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_perspective_desc* desc);

/* ---- Distance: the Euclidean distance to a shape, capped at a radius, through a linear ramp (DESIGN.md 5.20 "Distance rule") ----
 * Round outlines, inner and outer strokes of fractional width, dilate and erode by a DISC, glows with a defined falloff, signed
 * distance fields of a cached layer -- one function of one quantity, without the image leaving the device.  The squared distance is
 * an integer, so the result is defined on values, and every implementation produces these bits (include/jello_distance.h states the
 * host half and the per-axis pieces, tests/distance_ref.py restates all of it from the set definition).
 *   arguments   channel: 0..3, which of R, G, B, A of the source is read.  threshold: binary32, finite.  which: JH_DISTANCE_OUTER = 0 |
 *               JH_DISTANCE_INNER = 1 | JH_DISTANCE_SIGNED = 2.  edge: JH_DISTANCE_EDGE_ZERO = 0 | JH_DISTANCE_EDGE_CLAMP = 1.
 *               max_distance: R, an integer in [1, JH_DISTANCE_MAX_RADIUS = 255].  scale, offset: binary32, finite.  color[4]:
 *               binary32, premultiplied, linear; any value (as jh_shadow's).  flags: bit 0, JH_DISTANCE_STRAIGHT.  The rectangle (x,
 *               y, width, height) of dst is written; width == height == 0 means the whole image (x and y are then ignored).
 *   seed        a texel of the image is a SEED iff its chosen channel, the f16 widened to binary32, is >= threshold.  The comparison
 *               is IEEE: a NaN is not a seed, and -0 >= +0 holds.  A source that was never written reads as transparent black.
 *   distance^2  integers.  CAP = (R + 1)^2.  Dout(X, Y) = min(CAP, min of (x - X)^2 + (y - Y)^2 over the seeds (x, y) of the image);
 *               Din(X, Y) the same over the non-seeds.  Under EDGE_ZERO every integer position outside the image is a non-seed, so
 *               an inner distance ends at the image's border (as an erode under JH_MORPH_EDGE_ZERO does); under EDGE_CLAMP the
 *               positions outside the image do not exist.  The IMAGE is the edge, not the rectangle: seeds outside the rectangle
 *               but inside the image count.  A feature farther than R in x or in y is at least CAP away, so a window of +-R and the
 *               whole plane give the same D.  THE RESULT IS DEFINED ON THE SET, NOT ON PASSES: columns then rows, a lower envelope
 *               and a brute-force window all give these bits, and the implementation is free to choose.
 *   distance    binary32; sqrtf is the correctly rounded IEEE square root.  OUTER: s = sqrtf((float)Dout).  INNER: s =
 *               sqrtf((float)Din).  SIGNED: a non-seed texel has s = sqrtf((float)Dout) - 0.5f, a seed texel s = 0.5f -
 *               sqrtf((float)Din): the zero crossing lies on the texel edge between the two classes.  Where D = CAP, s is 256 in
 *               OUTER and INNER and +255.5 (non-seed) or -255.5 (seed) in SIGNED for R = 255, R + 1 and +-(R + 0.5) in general:
 *               "farther than R".
 *   value       v = minNum(maxNum(fmaf(s, scale, offset), 0), 1).  An overflow to +-Inf is clamped.  No NaN can arise: s, scale and
 *               offset are finite, so the fused product-sum is a finite real rounded once.
 *   store       p = color v, one product per channel.  STRAIGHT: f16(p) per channel, round to nearest even.  Otherwise as fine,
 *               jh_composite and jh_shadow store: a_inv = 1.0f / maxNum(p.a, 1e-6f); (f16(p.r a_inv + 0.0f), f16(p.g a_inv + 0.0f),
 *               f16(p.b a_inv + 0.0f), f16(p.a + 0.0f)).
 * So OUTER with scale = -1, offset = w + 0.5 is the coverage of the shape dilated by a DISC of radius w -- w may be fractional, and
 * the edge has a ramp one texel wide; INNER with scale = 1, offset = 0.5 - w is the erode by that disc; SIGNED with scale =
 * 1 / (2 R), offset = 0.5 is the usual SDF texture.  A call written in four quadrant rectangles equals the whole-image call.  OUTER is
 * monotone in the seed set: more seeds never make a distance longer.  On an image of height 1 or width 1 the disc is the box, and
 * the step ramp (scale -1, offset R + 1) on a 0 / 1 mask is jh_morphology's STRAIGHT dilate of it, bit for bit.
 *
 * jh_distance_plan: what the call will do with desc on an image_w x image_h image -- the resolved rectangle, R, CAP, the number of
 * planes (2 for SIGNED, else 1), their columns (rectangle width + 2 R) and rows (rectangle height), and the bytes of scratch they
 * take (0 for an image without texels).  Host only, no context.  It is what a caller needs to know which eager call must precede a
 * capture.  JH_ERR_INVALID for a null argument, a descriptor the rule refuses or a rectangle the image refuses, plan then untouched.
 *
 * jh_distance: the rule applied to src_image_id, written to the rectangle of dst_image_id.  The images carry their own sizes and
 * must be JL_RGBA16_FLOAT and of equal size.  dst_image_id may equal src_image_id: the source is read once into the intermediate and
 * no pass reads what the call has written.  Texels of dst outside the rectangle keep their bits; a dst that was never written is
 * cleared to transparent black first and then counts as written.
 * Stream-ordered on the context's stream, never waits: TWO kernel launches (the columns' run lengths into planes of uint16_t; the
 * rows' lower envelope over them from LDS, the square root, the ramp and the store), plus a fill when dst has to be cleared.  The
 * row pass's walk stops as soon as dx^2 reaches the best squared distance so far, so its cost follows the distance found, not R.
 * The planes live in a scratch array of the context, planes x rect height x (rect width + 2 R) x 2 bytes, which only grows: the call
 * may be captured between jh_graph_begin and jh_graph_end once a call needing no more has run eagerly (a capture that would have to
 * grow it is refused with JH_ERR_OOM and that advice).  With profiling on the call is a query "distance" with stage = -1 in
 * jh_profile_collect_tree.  Not in band mode (jh_set_band): the rows next to a band belong to another rank's context.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_distance: ": a
 * null desc; an unknown source or destination id; an image that is not RGBA16F; images of different size; an unknown channel,
 * which, edge or flag bit; max_distance 0 or above 255; a threshold, scale or offset that is not finite; a rectangle that is not
 * inside the image or that is empty in exactly one dimension; a band set with jh_set_band. */
typedef enum jh_distance_which { JH_DISTANCE_OUTER = 0, JH_DISTANCE_INNER = 1, JH_DISTANCE_SIGNED = 2 } jh_distance_which;
typedef enum jh_distance_edge { JH_DISTANCE_EDGE_ZERO = 0, JH_DISTANCE_EDGE_CLAMP = 1 } jh_distance_edge;
#define JH_DISTANCE_STRAIGHT 1u
#define JH_DISTANCE_MAX_RADIUS 255u
typedef struct jh_distance_desc {
    int channel;                   /* 0..3: R, G, B, A of the source */
    float threshold;               /* a texel is a seed iff its channel >= threshold */
    int which;                     /* jh_distance_which */
    int edge;                      /* jh_distance_edge */
    uint32_t max_distance;         /* R, 1..255 */
    float scale, offset;           /* v = clamp(fmaf(s, scale, offset), 0, 1) */
    float color[4];                /* premultiplied, linear */
    uint32_t flags;                /* bit 0: JH_DISTANCE_STRAIGHT */
    uint32_t x, y, width, height;  /* rectangle of dst that is written; 0 x 0: the whole image */
} jh_distance_desc;
typedef struct jh_dist_plan {
    uint32_t x, y, width, height;  /* the resolved rectangle */
    uint32_t radius, cap;          /* R and (R + 1)^2 */
    uint32_t planes;               /* 1, or 2 for SIGNED */
    uint32_t plane_columns, plane_rows; /* width + 2 R, height */
    uint32_t reserved;             /* 0 */
    uint64_t scratch_bytes;        /* planes x plane_rows x plane_columns x 2; 0 for an image without texels */
} jh_dist_plan;
int jh_distance_plan(const jh_distance_desc* desc, uint32_t image_w, uint32_t image_h, jh_dist_plan* plan);
int jh_distance(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, const jh_distance_desc* desc);

/* ---- load: 8-bit surfaces and 8-bit Y'CbCr 4:2:0 frames INTO RGBA16F images (DESIGN.md 5.21 "Load rule") ----
 * The inverses of jh_blit and jh_blit_yuv: a decoded picture or video frame in device memory becomes an image every image call
 * takes.  The result is defined byte for byte (include/jello_load.h is the rule's text for the kernels, the queries and their host
 * twin; tests/load_ref.py restates it in numpy):
 *   texel     from four 8-bit codes (r, g, b, a) and a transfer:  U(c) = the binary32 nearest to c / 255 (= (float)c / 255.0f);
 *             L(c) = kSrgbToLinear[c], the decode table of the fine kernel.  Colour = L(c) under an sRGB format or transfer, U(c)
 *             otherwise; alpha is always U(a).
 *               JH_LOAD_ALPHA_STRAIGHT        texel_pack(colour, U(a)): RGBA16F images hold straight colour
 *               JH_LOAD_ALPHA_PREMULTIPLIED   texel_unpremultiply(colour, U(a)), the store rule of DESIGN.md 5.8 (what jh_blit
 *                                             writes is premultiplied); a = 0 under a non-zero colour gives large values or Inf
 *               JH_LOAD_ALPHA_OPAQUE          byte 3 is ignored, alpha is 1.0 (BGRX surfaces)
 *             BGRA formats swap bytes 0 and 2.
 *   chroma    planes are ceil(w / 2) x ceil(h / 2), laid out as jh_blit_yuv writes them, sample (cx, cy) at luma position
 *             (2 cx + 1/2, 2 cy + 1/2).  For the texel (x, y) of the frame: cx0 = x >> 1, cx1 = clamp(cx0 + (x odd ? 1 : -1), 0,
 *             ceil(w / 2) - 1), cy0 and cy1 the same in y.  The sum S is 16 x a code:
 *               JH_CHROMA_REPLICATE  S = 16 C[cy0][cx0]   (the adjoint of jh_blit_yuv's box)
 *               JH_CHROMA_BILINEAR   S = 9 C[cy0][cx0] + 3 C[cy0][cx1] + 3 C[cy1][cx0] + C[cy1][cx1]   (the edge sample repeated)
 *   codes     in integers, with Y' = Y - o (o = 16 limited, 0 full), u = S_cb - 2048, v = S_cr - 2048, the shift arithmetic:
 *               R = clamp8((16 Ky Y' + Krv v         + 2^19) >> 20)
 *               G = clamp8((16 Ky Y' + Kgu u + Kgv v + 2^19) >> 20)
 *               B = clamp8((16 Ky Y' + Kbu u         + 2^19) >> 20)
 *   tables    round-half-even(exact * 2^16) of 255/219 or 1, 2 (1 - Kr) s, -2 Kb (1 - Kb) / Kg s, -2 Kr (1 - Kr) / Kg s, 2 (1 - Kb) s,
 *             s = 255/224 or 1 (jello_amd/csrc/load_decode_lut.h, tools/gen_load_tables.py).   (Ky | Krv | Kgu, Kgv | Kbu)
 *               BT.601 limited   76309 | 104597 | -25675, -53279 | 132201
 *               BT.601 full      65536 |  91881 | -22553, -46802 | 116130
 *               BT.709 limited   76309 | 117489 | -13975, -34925 | 138438
 *               BT.709 full      65536 | 103206 | -12276, -30679 | 121609
 *             The codes are within 0.51 of the real-valued inverse matrix, clamped; every grey gives R = G = B.
 *   yuv texel the texel rule on (R, G, B, 255) with the transfer, straight: what jh_load_surface (OPAQUE) makes of those codes.
 *
 * jh_load_texel and jh_load_yuv_codes: the rule on batches, host only, no context.  jh_load_texel: format_or_transfer is a
 * jh_surface_format, or 4 + a jh_yuv_transfer for RGBA-ordered codes under that transfer; rgba holds n pixels of 4 bytes, out gets
 * 4 n f16 bit patterns (r, g, b, a).  jh_load_yuv_codes: y holds n codes, s_cb and s_cr n sums in [0, 4080], rgb gets 3 n codes.
 * JH_ERR_INVALID for a null argument or an unknown enum value (or a sum above 4080), the outputs then untouched.
 *
 * jh_load_surface: the frame at desc->src -- height rows of 4 * width bytes, desc->pitch apart, in desc->format -- into the rectangle
 * (x, y, width, height) of dst_image_id; 0 x 0 names the whole image, and the frame has the rectangle's size.  jh_load_yuv: the same
 * for the planes of a width x height 4:2:0 frame.  dst must be JL_RGBA16_FLOAT.  Texels outside the rectangle keep their bits; a dst
 * that was never written is cleared to transparent black first (where the rectangle is not the whole image) and then counts as
 * written.  The source is only read, and never between a row's bytes and its pitch; any pointer and any pitch >= the row's bytes is
 * legal.  Source memory that overlaps the destination image's is undefined.
 * Stream-ordered on the context's stream, never waits: ONE kernel launch (plus the fill), no scratch, no resident tables: always
 * capturable between jh_graph_begin and jh_graph_end (the graph then holds the pointers).  With profiling on each call is one
 * query, "load_surface" or "load_yuv", with stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band).
 * JH_ERR_INVALID, with nothing enqueued, each with a message that starts "jh_load_surface: " or "jh_load_yuv: ": a null desc; an
 * unknown destination id or one that is not RGBA16F; a rectangle that is not inside the image or empty in exactly one dimension; an
 * unknown format, alpha, layout, matrix, range, transfer or chroma; a null src or required plane; a pitch below the row's bytes; a
 * band set with jh_set_band. */
typedef enum jh_load_alpha { JH_LOAD_ALPHA_STRAIGHT = 0, JH_LOAD_ALPHA_PREMULTIPLIED = 1, JH_LOAD_ALPHA_OPAQUE = 2 } jh_load_alpha;
typedef enum jh_chroma_filter { JH_CHROMA_REPLICATE = 0, JH_CHROMA_BILINEAR = 1 } jh_chroma_filter;
typedef struct jh_load_surface_desc {
    int32_t format, alpha;         /* jh_surface_format, jh_load_alpha */
    const void* src;               /* caller-owned device memory */
    uint64_t pitch;                /* bytes between the rows */
    uint32_t x, y, width, height;  /* rectangle of dst that is written = the frame's size; 0 x 0: the whole image */
} jh_load_surface_desc;
typedef struct jh_load_yuv_desc {
    int32_t layout, matrix, range, transfer; /* jh_yuv_layout, jh_yuv_matrix, jh_yuv_range, jh_yuv_transfer */
    int32_t chroma, reserved;                /* jh_chroma_filter; 0 */
    const void* plane[3];                    /* caller-owned device memory, as jh_yuv_desc's */
    uint64_t pitch[3];                       /* bytes between the rows of each plane */
    uint32_t x, y, width, height;            /* rectangle of dst that is written = the frame's size; 0 x 0: the whole image */
} jh_load_yuv_desc;
int jh_load_texel(int format_or_transfer, int alpha, uint64_t n, const uint8_t* rgba, uint16_t* out);
int jh_load_yuv_codes(int matrix, int range, uint64_t n, const uint8_t* y, const uint16_t* s_cb, const uint16_t* s_cr, uint8_t* rgb);
int jh_load_surface(jh_ctx* ctx, uint64_t dst_image_id, const jh_load_surface_desc* desc);
int jh_load_yuv(jh_ctx* ctx, uint64_t dst_image_id, const jh_load_yuv_desc* desc);

/* ---- Stats: content bounds, channel extremes and histograms of an RGBA16F image (DESIGN.md 5.22 "Stats rule") ----
 * The one image call that brings a fact about an image OUT: the box of a layer's content (the rectangle every other image call
 * takes), the channel extremes and four 256-bin histograms (what chooses jh_color_filter's LINEAR / TABLE parameters: auto-levels,
 * normalisation, equalisation), as a fixed-size record in caller-owned device memory.  Everything in the record is an integer count
 * or an integer min / max over the SET of texels of the rectangle, so it is defined byte for byte whatever the decomposition
 * (include/jello_stats.h is the rule's text for the kernels, the library, the host twin and the stand-alone check;
 * tests/stats_ref.py restates it in numpy):
 *   content     a texel is CONTENT iff its chosen channel (0..3), the f16 widened to binary32, is >= threshold -- jh_distance's seed
 *               test: IEEE, a NaN is not content, -0 >= +0 holds; the threshold is finite.  A source that was never written reads
 *               as transparent black.  content_count: the content texels of the rectangle; always written.
 *   bounds      (JH_STATS_BOUNDS) x0, y0, x1, y1: the smallest box of the content texels INSIDE the rectangle -- texels outside it
 *               do not exist for this call -- in IMAGE coordinates, x1 and y1 exclusive; 0, 0, 0, 0 without content.
 *   population  the texels the extremes and the histogram are taken over: JH_STATS_ALL: every texel of the rectangle;
 *               JH_STATS_CONTENT: the content texels only (a layer on a transparent background).  population_count and nan_count
 *               are written when EXTREMES or HISTOGRAM is asked for.
 *   extremes    (JH_STATS_EXTREMES) per channel, over the population's non-NaN values, under the order of jh_morphology
 *               (totalOrder: -Inf < ... < -0 < +0 < ... < +Inf), as f16 bit patterns.  A channel without a non-NaN value has
 *               min_bits = 0x7C00 and max_bits = 0xFC00, the neutral elements.  nan_count[c]: the NaNs of channel c in the
 *               population; they take no other part in the extremes.
 *   histogram   (JH_STATS_HISTOGRAM) the code of a value v (straight colour: nothing is multiplied by alpha): q = the clamp of
 *               jh_blit (NaN -> 0, -0 -> +0, +Inf -> 1);  JH_STATS_LINEAR: rintf(q * 255.0f) -- the product is exact for an f16, so
 *               this is round-half-even of 255 q;  JH_STATS_SRGB: the code u with t[u] <= q < t[u + 1] of jh_blit's threshold table
 *               (jello_amd/csrc/srgb_encode_lut.h), code 0 from 0 and code 255 up to 1.  `transfer` is the code of R, G, B; alpha is
 *               always LINEAR.  A NaN counts in bin 0 AND in nan_count.  Each channel's 256 bins sum to population_count.
 *   parts       a part that `what` does not ask for is written as zeros (min_bits and max_bits too: zeros, not the neutral
 *               elements).  An image without texels (the 0 x 0 rectangle of an image of no width or height) writes a record of
 *               zeros with the eight header words filled in: there is no texel to be an extreme.
 * The record of a rectangle is the merge -- integer sums, mins, maxes, the union of the boxes -- of the records of any disjoint
 * rectangles that tile it: four quadrant calls merged equal one call (jello_amd.stats.merge).
 *
 * jh_stats_plan: what the call will do with desc on an image_w x image_h image -- the resolved rectangle, the kernel launches (2; 1
 * for an image without texels), the bytes of the record (sizeof(jh_stats_record)) and the bytes of scratch the call keeps (0 for an
 * image without texels; otherwise JH_STATS_MAX_PARTIALS partial records, the same for every image: what a device of 256 compute
 * units uses).  Host only, no context.  JH_ERR_INVALID for a null argument, a descriptor the rule refuses or a rectangle the image
 * refuses, plan then untouched.
 * jh_stats_codes: the histogram code of n f16 bit patterns under `transfer`, host only, no context.  JH_ERR_INVALID for a null
 * argument (with n > 0) or an unknown transfer, codes then untouched.
 *
 * jh_stats: the record of the rectangle of src_image_id into out_device_ptr, sizeof(jh_stats_record) bytes of caller-owned device
 * memory on an 8-byte boundary.  The source is only read: the call never clears an image or marks it as written.
 * Stream-ordered on the context's stream, never waits: TWO kernel launches with the kernel boundary as the only hand-off -- every
 * workgroup of the first streams its share of the rectangle and writes one partial record (box, extremes and counts reduced in
 * registers, across the wave and through LDS; the bins in LDS) to its own slot of a scratch array; the second combines the
 * partials in a fixed order and writes every byte of the record.  No global atomics, no fill.  The scratch array has one size for
 * every image and only grows: the call may be captured between jh_graph_begin and jh_graph_end once one call has run eagerly (a
 * capture that would have to allocate it is refused with JH_ERR_OOM and that advice).  With profiling on the call is a query
 * "stats" with stage = -1 in jh_profile_collect_tree.  Not in band mode (jh_set_band): the rows outside a band belong to another
 * rank's context.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_stats: ": a null
 * desc or out pointer; an out pointer that is not 8-byte aligned; an unknown image id; an image that is not RGBA16F; `what` 0 or
 * with an unknown bit; an unknown channel, population or transfer; a threshold that is not finite; a rectangle that is not inside
 * the image or that is empty in exactly one dimension; a rectangle of more than JH_STATS_MAX_TEXELS = 2^31 texels (every count then
 * fits a uint32_t); a band set with jh_set_band. */
typedef enum jh_stats_population { JH_STATS_ALL = 0, JH_STATS_CONTENT = 1 } jh_stats_population;
typedef enum jh_stats_transfer { JH_STATS_LINEAR = 0, JH_STATS_SRGB = 1 } jh_stats_transfer;
#define JH_STATS_BOUNDS 1u
#define JH_STATS_EXTREMES 2u
#define JH_STATS_HISTOGRAM 4u
#define JH_STATS_MAX_TEXELS 2147483648u /* 2^31: every count fits a uint32_t */
#define JH_STATS_MAX_PARTIALS 1024u     /* partial records of the scratch array: 4 workgroups to each of 256 compute units */
typedef struct jh_stats_desc {
    uint32_t what;                 /* any non-empty subset of JH_STATS_BOUNDS | JH_STATS_EXTREMES | JH_STATS_HISTOGRAM */
    int channel;                   /* 0..3: the channel of the content test */
    float threshold;               /* content: the texels whose channel is >= threshold */
    int population;                /* jh_stats_population: which texels the extremes and the histogram are taken over */
    int transfer;                  /* jh_stats_transfer: the histogram's code for R, G, B; alpha is always LINEAR */
    uint32_t x, y, width, height;  /* rectangle of src that is read; 0 x 0: the whole image */
} jh_stats_desc;
typedef struct jh_stats_record {
    uint32_t x, y, width, height;                  /* the resolved rectangle */
    uint32_t what, population, transfer, reserved; /* of the descriptor; 0 */
    uint32_t content_count;                        /* content texels in the rectangle */
    uint32_t bounds[4];                            /* x0, y0, x1, y1 in IMAGE coordinates, x1 / y1 exclusive; 0, 0, 0, 0 when content_count == 0 */
    uint32_t population_count;                     /* texels that took part in extremes and histogram */
    uint32_t nan_count[4];                         /* per channel, over the population */
    uint16_t min_bits[4], max_bits[4];             /* f16 bit patterns */
    uint32_t histogram[4][256];
} jh_stats_record;
typedef struct jh_stats_plan_t {
    uint32_t x, y, width, height;  /* the resolved rectangle */
    uint32_t launches, reserved;   /* 2, or 1 for an image without texels; 0 */
    uint64_t record_bytes;         /* sizeof(jh_stats_record) */
    uint64_t scratch_bytes;        /* 0 for an image without texels, else JH_STATS_MAX_PARTIALS partial records */
} jh_stats_plan_t;
int jh_stats_plan(const jh_stats_desc* desc, uint32_t image_w, uint32_t image_h, jh_stats_plan_t* plan);
int jh_stats_codes(int transfer, uint64_t n, const uint16_t* f16_bits, uint8_t* codes);
int jh_stats(jh_ctx* ctx, uint64_t src_image_id, const jh_stats_desc* desc, void* out_device_ptr);

/* ---- 3D LUT: a colour lookup table applied to an RGBA16F image by tetrahedral interpolation (DESIGN.md 5.23 "LUT rule") ----
 * What jh_color_filter cannot say -- a .cube grade, a gamut map, a film look, anything that mixes the channels non-linearly -- and a
 * way to BAKE a chain of colour calls into one pass: the table is an ordinary RGBA16F image of the context, so every image call can
 * write it; a sequence of jh_color_filter calls over an identity table leaves a table that applies the whole chain, per texel, in
 * one launch.  The reference project has no counterpart; the result is defined here on values, byte for byte
 * (include/jello_lut3d.h is the rule's text for the kernel, the library, the host twin and the stand-alone check;
 * tests/lut3d_ref.py restates it in numpy):
 *   the LUT   an RGBA16F image of the context, N texels wide and N^2 high, 2 <= N <= 65.  Entry (i, j, k) indexes (red, green, blue)
 *             and is the texel (x = i, y = j + N k): red varies fastest, the .cube order.  Its r, g, b are the output colour for
 *             the input (i, j, k) / (N - 1); its alpha is ignored.  A never-written LUT reads as zeros, like every never-written
 *             source.  There is no scratch slot, no resident key and no staleness rule: the call is always capturable.
 *   per texel binary32, nothing contracted but the stated fmaf; h_c is the stored (un-premultiplied) f16 of channel c, widened.
 *     1 clamp     c = h > 0 ? h : 0; c = c < 1 ? c : 1 -- compare and select, so NaN and -0 become +0, as in the colour filter.
 *     2 position  p = c (N - 1), k = min((int)p, N - 2), f = p - (float)k.  Every one of these operations is exact for every f16
 *                 input and every legal N: p, f, 1 - f and the differences of two fractions are representable in binary32.  The
 *                 position carries no rounding, and the weights below sum to exactly 1.
 *     3 walk      start at the vertex V0 = (k_r, k_g, k_b) and step +1 along one axis at a time in descending order of the
 *                 fractions: V1, V2 and V3 = (k_r + 1, k_g + 1, k_b + 1).  Ties go r before g before b: the order is the stable
 *                 sort decided by f_r >= f_g, f_r >= f_b, f_g >= f_b.  With the fractions f1 >= f2 >= f3 in that order the weights
 *                 are w0 = 1 - f1, w1 = f1 - f2, w2 = f2 - f3, w3 = f3, all exact.
 *     4 sum       per colour channel: m = w0 V0.c, then m = fmaf(w1, V1.c, m), m = fmaf(w2, V2.c, m), m = fmaf(w3, V3.c, m) -- one
 *                 multiply and three fmaf, in this order.  Zero weights are multiplied, not skipped: 0 x Inf is NaN, as for
 *                 jh_convolve.  The tie rule therefore decides which vertex a zero weight touches, which non-finite entries show
 *                 and nothing else does.
 *     5 store     f16(m), round to nearest even; a NaN result is any NaN.  Alpha is the source's bit pattern, copied.
 * So: an identity table whose N - 1 is a power of two returns every finite f16 in [0, 1] bit for bit (-0 becomes +0, values
 * outside are clamped, NaN becomes 0); exactly four entries are read per texel; alpha never changes.
 *
 * jh_lut3d_identity: the identity table of n into out_texels, n^3 entries of four f16 bit patterns in the image's order: entry
 * value f16(i / (n - 1)), rounded once from binary64, alpha 1.0.  jh_lut3d_texels: the rule on `count` texels (in_texels, four f16
 * bit patterns each) over a host table lut_texels of n^3 entries, into out_texels.  Host only, no context.  JH_ERR_INVALID for a
 * null argument (jh_lut3d_texels: with count > 0, the table always) or an n outside 2..65, the outputs then untouched.
 *
 * jh_lut3d: the rule applied to the rectangle (x, y, width, height) of src_image_id through the table lut_image_id, written to the
 * same rectangle of dst_image_id; one rectangle for both, 0 x 0: the whole source.  src == dst is legal (the rule is per texel) and
 * so is lut == src.  A never-written source reads as transparent black; a never-written destination is cleared outside the
 * rectangle and the context's generation moves, as for jh_color_filter.  Stream-ordered on the context's stream, never waits: one
 * kernel launch (tables of N <= 17 are copied into LDS by every workgroup, larger ones are gathered from memory).  May be captured
 * between jh_graph_begin and jh_graph_end at any time.  With profiling on the call is a query "lut3d" with stage = -1 in
 * jh_profile_collect_tree.  Not in band mode (jh_set_band): a band's rows are one rank's, the table the context's.
 * JH_ERR_INVALID, with nothing enqueued, no memory touched and nothing flushed, each with a message that starts "jh_lut3d: ": a null
 * desc; an unknown source, destination or LUT id; an image that is not RGBA16F; a size outside 2..65; flags that are not 0; a LUT
 * image that is not exactly size x size^2; the LUT being the destination; a rectangle that is not inside the source or the
 * destination or that is empty in exactly one dimension; a band set with jh_set_band. */
#define JH_LUT3D_MIN_SIZE 2u
#define JH_LUT3D_MAX_SIZE 65u
typedef struct jh_lut3d_desc {
    uint32_t size;                 /* N: the LUT image is N x N^2 */
    uint32_t flags;                /* must be 0 */
    uint32_t x, y, width, height;  /* rectangle of src that is read and of dst that is written; 0 x 0: the whole source */
} jh_lut3d_desc;
int jh_lut3d_identity(uint32_t n, uint16_t* out_texels);
int jh_lut3d_texels(uint32_t n, const uint16_t* lut_texels, const uint16_t* in_texels, uint64_t count, uint16_t* out_texels);
int jh_lut3d(jh_ctx* ctx, uint64_t src_image_id, uint64_t dst_image_id, uint64_t lut_image_id, const jh_lut3d_desc* desc);

/* ---- profiling ---- */
int jh_profile_enable(jh_ctx* ctx, int on);
/* Waits for the device, writes up to max records (one per dispatch since the last collect), returns the count. */
int jh_profile_collect(jh_ctx* ctx, jh_profile_record* out, int max);
/* Nested spans as in the reference's profiler: group_begin opens a group under the innermost open one (Profiler.Start at
 * top level, ProfilerGroup.Nest below), group_end closes it; every dispatch issued in between becomes a query of that
 * group.  No-ops while profiling is disabled (the reference's nil profiler).  collect_tree = Profiler.Collect: waits for
 * the device and returns everything since the last collect as a flattened tree (and clears it, like jh_profile_collect). */
int jh_profile_group_begin(jh_ctx* ctx, const char* label);
int jh_profile_group_end(jh_ctx* ctx);
int jh_profile_collect_tree(jh_ctx* ctx, jh_profile_node* out, int max);

/* ---- diagnostics (not used by the render path) ----
 * Evaluates one of the kernels' scalar math routines on n host floats: op 0 sin, 1 cos, 2 atan2(a,b),
 * 3 acos, 4 asin, 5 |a|^(2/3), 6 a/b, 7 sqrt, 8 round-to-even, 9 u32(a), 10 i32(a), 11 f32->f16 bits,
 * 12 a*b+a (uncontracted), 13 floor(a*b+0.5), 14 min(a,b), 15 max(a,b), 16 clamp(a,0,1), 17 clamp(a*b,0,1). */
int jh_selftest_math(jh_ctx* ctx, int op, const float* a, const float* b, float* out, uint32_t n);
/* Runs the allocation patterns the kernels rely on -- a returning atomic add with a different value per lane on one address, inside
 * a loop that lanes skip and leave at different trips -- on n_waves waves (1..4096) and compares with a serial execution on the
 * host: form 0 the plain per-lane atomic (what the compiler's atomic optimizer makes of it), 1 the hand-aggregated wave_bump
 * (kcommon.h) the hot call sites use, 2 the wave-private LDS forms (XOR into one word, 64-bit OR into a word per lane).
 * Returns 0 when everything agrees, the number of violations (> 0) otherwise, a negative jh_status on misuse / device errors.
 * (Round 5 met a compiler strategy that returned overlapping ranges for form 0; tests/test_gpu_math.py runs all three.) */
int jh_selftest_atomics(jh_ctx* ctx, int form, uint32_t seed, uint32_t n_waves);
/* Fills every per-context scratch allocation (the count / offset arrays and counters of the deterministic allocators)
 * with `byte` and forgets that any counter was left clean -- the state of freshly allocated device memory that happens
 * not to be zero.  Tests use it to show that no stage relies on what an earlier frame (or hipMalloc) left behind, the
 * way the reference's pooled buffers hold stale data (engine/wgpu_engine/wgpu.go:772-808). */
uint64_t jh_debug_scratch_bytes(jh_ctx* ctx, int slot);   /* capacity of an internal scratch array (tests); slot -1: all of them */
/* Internal scratch arrays (count / offset arrays of the deterministic allocators, flatten's temporary) grow on demand and are
   kept.  jh_scratch_trim waits for the stream and frees them all: after one frame that was much larger than the ones to come,
   or after a first attempt with the estimator's generous bump sizes (the reference's pool keeps its buffers in the same way,
   wgpu.go:601-616; this is the counterpart of dropping that pool).  Captured graphs become stale. */
int jh_scratch_trim(jh_ctx* ctx);
/* tests: bit 0 = every wave of flatten starts in region 0 of its temporary, bit 1 = always eight regions (kernels_flatten.hip,
   FlTemp): ordinary scenes then fill regions up and move on, which the product only does close to the line buffer's capacity;
   bit 2 = a batch of more than 48 lines allocates its slots job by job (the product: more than 51 200);
   bit 3 = k_flatten_items runs as ONE workgroup: four waves and one unit counter, so that the item counts at which its work
   distribution changes (a unit of 64 filled exactly, one item more, heavy items only, ...) are scenes of a few hundred shapes */
int jh_debug_flatten_regions(jh_ctx* ctx, uint32_t flags);
uint64_t jh_debug_graph_self_cleans(jh_ctx* ctx);  /* replays that had to zero an internal counter first (tests) */
int jh_debug_poison_scratch(jh_ctx* ctx, int byte);
/* tests and timing: which instantiation jh_lut3d launches -- 0 the launcher's choice (tables of N <= 17 in LDS), 1 always gathered
   from memory, 2 always from LDS (a call with a larger table is then refused).  The results do not depend on it. */
int jh_debug_lut3d_variant(jh_ctx* ctx, int variant);
/* tests: one launch of the single-pass exclusive u32 scan that flatten, path_count and jh_dash allocate through, on the context's
   stream and scratch: out[i] = in[0] + in[stride] + ... + in[(i - 1) stride] mod 2^32 for i < n.  `in_id` and `out_id` are context
   buffers of at least n_max * stride and n_max words.  n = n_max, or min(n_max, word `count_word` of the buffer `count_id`) when
   count_id != 0: the count is read on the device.  With total_id != 0 the sum of the n inputs goes to word `total_word` of that
   buffer.  Words of `out` from n on are not written.  Stream-ordered and capturable (after one eager call of at least this n_max);
   JH_ERR_INVALID for an unknown id, a buffer that is too small or a stride of 0. */
int jh_debug_scan_u32(jh_ctx* ctx, uint64_t in_id, uint64_t out_id, uint32_t stride, uint32_t n_max, uint64_t count_id, uint32_t count_word,
                      uint64_t total_id, uint32_t total_word);

/* ---- introspection ---- */
int jh_device_info(jh_ctx* ctx, char* name, int name_len, int* compute_units, uint64_t* total_mem);
uint64_t jh_pool_bytes(jh_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* JELLO_HIP_H */
