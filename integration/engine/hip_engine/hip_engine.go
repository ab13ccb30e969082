// Package hip_engine replays renderer.Recordings on an AMD MI355X (gfx950) through libjello_hip.so.
//
// It is the drop-in replacement for engine/wgpu_engine on the compute path: Scene, encoding and
// renderer stay as they are; this package walks the Recording exactly like
// wgpu_engine.Engine.RunRecording (engine/wgpu_engine/wgpu.go:322-643) and forwards every command to
// the C ABI of include/jello_hip.h.  Drop this directory into the reference tree as
// engine/hip_engine/ (adjust the two #cgo paths) and apply integration/renderer_bump_sizes.patch.
//
// NOT COMPILED in the repository it comes from (the build image has no Go toolchain); the C++ twin
// jello_amd/host/hip_engine.cpp makes the same calls in the same order and is what the tests run.
package hip_engine

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../jello_amd -ljello_hip
#include <stdlib.h>
#include "jello_hip.h"
*/
import "C"

import (
	"encoding/binary"
	"fmt"
	"image"
	"runtime"
	"unsafe"

	"honnef.co/go/jello/encoding"
	"honnef.co/go/jello/mem"
	"honnef.co/go/jello/profiler"
	"honnef.co/go/jello/renderer"
)

type Engine struct {
	ctx         *C.jh_ctx
	renderer    *renderer.Renderer
	resolver    *renderer.Resolver
	fullShaders *renderer.FullShaders
	downloads   map[renderer.ResourceID][]byte
	target      *targetTexture // RenderToSurface's RGBA16F target (eng.target, lib.go:279-284)
}

// SurfaceFormat is RendererOptions.SurfaceFormat (lib.go:19-22): the 8-bit format RenderToSurface writes
// (jh_surface_format; the conversion rule is in include/jello_hip.h).
type SurfaceFormat int

const (
	SurfaceRGBA8Unorm SurfaceFormat = C.JH_SURFACE_RGBA8_UNORM
	SurfaceBGRA8Unorm SurfaceFormat = C.JH_SURFACE_BGRA8_UNORM
	SurfaceRGBA8Srgb  SurfaceFormat = C.JH_SURFACE_RGBA8_SRGB
	SurfaceBGRA8Srgb  SurfaceFormat = C.JH_SURFACE_BGRA8_SRGB
)

// YUVFormat selects what RenderToYUV writes (jh_yuv_layout, jh_yuv_matrix, jh_yuv_range, jh_yuv_transfer; the conversion
// rule is in include/jello_hip.h, "YUV blit").
type YUVFormat struct {
	Layout, Matrix, Range, Transfer int
}

const (
	YUVNV12         = C.JH_YUV_NV12
	YUVI420         = C.JH_YUV_I420
	YUVBT601        = C.JH_YUV_BT601
	YUVBT709        = C.JH_YUV_BT709
	YUVLimited      = C.JH_YUV_LIMITED
	YUVFull         = C.JH_YUV_FULL
	YUVTransferNone = C.JH_YUV_TRANSFER_NONE
	YUVTransferSrgb = C.JH_YUV_TRANSFER_SRGB
)

// surfaceTargetID names the target's buffer on the context: recordings take their ResourceIDs from a counter that starts at 1
// (recording.go:15-19) and never reaches the top bit.
const surfaceTargetID renderer.ResourceID = 1<<63 | 0x7461726765740000

// targetTexture: a context buffer of Width*Height RGBA16F pixels (lib.go:200-226 newTargetTexture).
type targetTexture struct {
	id            renderer.ResourceID
	ptr           unsafe.Pointer
	Width, Height uint32
}

// New mirrors wgpu_engine.New (wgpu.go:157-178).  device is the HIP device ordinal; one Engine per
// GPU, engines on different GPUs are independent.
func New(device int) (*Engine, error) {
	var ctx *C.jh_ctx
	if rc := C.jh_create(&ctx, C.int(device)); rc != C.JH_OK {
		return nil, fmt.Errorf("jh_create: %d", int(rc))
	}
	// ShaderIDs are the jh_stage values, i.e. the FullShaders field order (render.go:17-43).
	fs := &renderer.FullShaders{
		PathtagReduce: C.JH_PATHTAG_REDUCE, PathtagReduce2: C.JH_PATHTAG_REDUCE2, PathtagScan1: C.JH_PATHTAG_SCAN1,
		PathtagScanSmall: C.JH_PATHTAG_SCAN_SMALL, PathtagScanLarge: C.JH_PATHTAG_SCAN_LARGE, BboxClear: C.JH_BBOX_CLEAR,
		Flatten: C.JH_FLATTEN, DrawReduce: C.JH_DRAW_REDUCE, DrawLeaf: C.JH_DRAW_LEAF, ClipReduce: C.JH_CLIP_REDUCE,
		ClipLeaf: C.JH_CLIP_LEAF, Binning: C.JH_BINNING, TileAlloc: C.JH_TILE_ALLOC, BackdropDyn: C.JH_BACKDROP_DYN,
		PathCountSetup: C.JH_PATH_COUNT_SETUP, PathCount: C.JH_PATH_COUNT, Coarse: C.JH_COARSE,
		PathTilingSetup: C.JH_PATH_TILING_SETUP, PathTiling: C.JH_PATH_TILING, FineArea: C.JH_FINE_AREA,
		FineMSAA8: C.JH_FINE_MSAA8, FineMSAA16: C.JH_FINE_MSAA16,
		// PathtagIsCPU stays false: the three-level scan stages exist on the HIP side.
	}
	return &Engine{ctx: ctx, renderer: renderer.New(), resolver: renderer.NewResolver(), fullShaders: fs,
		downloads: map[renderer.ResourceID][]byte{}}, nil
}

func (e *Engine) Close() { C.jh_destroy(e.ctx) }

// The reference panics on every misuse (wgpu.go:77,213,282,544,558,594,955); the C ABI returns
// codes, which become panics here to keep the calling convention of wgpu_engine.
func (e *Engine) check(rc C.int, what string) {
	if rc != C.JH_OK {
		panic(fmt.Sprintf("hip_engine: %s: %s", what, C.GoString(C.jh_last_error(e.ctx))))
	}
}

// ExternalImage hands the engine a caller-owned device allocation for an ImageProxy (wgpu.go:90-93,
// lib.go:257-262): width*height*8 bytes of device memory for the RGBA16F target.
type ExternalImage struct {
	Proxy     renderer.ImageProxy
	DevicePtr unsafe.Pointer
}

// RunRecording mirrors wgpu.go:322-643.  Frees are deferred to the end of the recording
// (wgpu.go:601-616); buffers the recording never frees stay resident (wgpu.go:631-640).
func (e *Engine) RunRecording(rec renderer.Recording, external []ExternalImage, pgroup string) {
	label := C.CString(pgroup) // pgroup = pgroup.Nest("RunRecording"), wgpu.go:330: a no-op unless jh_profile_enable(1)
	defer C.free(unsafe.Pointer(label))
	e.check(C.jh_profile_group_begin(e.ctx, label), "profile_group_begin")
	defer C.jh_profile_group_end(e.ctx)

	for _, x := range external {
		e.check(C.jh_image_import(e.ctx, C.uint64_t(x.Proxy.ID), x.DevicePtr, C.uint32_t(x.Proxy.Width),
			C.uint32_t(x.Proxy.Height), C.int(x.Proxy.Format)), "image_import")
	}
	var freeBufs, freeImages []renderer.ResourceID
	pendingClears := map[renderer.ResourceID]bool{}
	for _, cmd := range rec.Commands {
		switch cmd := cmd.(type) {
		case *renderer.Upload:
			e.upload(cmd.Buffer.ID, cmd.Data)
		case *renderer.UploadUniform:
			e.upload(cmd.Buffer.ID, cmd.Data)
		case *renderer.UploadImage:
			p := cmd.Proxy
			e.check(C.jh_image_upload(e.ctx, C.uint64_t(p.ID), C.uint32_t(p.Width), C.uint32_t(p.Height), C.int(p.Format),
				unsafe.Pointer(unsafe.SliceData(cmd.Data)), C.uint64_t(len(cmd.Data))), "image_upload")
		case *renderer.WriteImage: // wgpu.go:422-452
			p := cmd.Proxy
			if C.jh_image_device_ptr(e.ctx, C.uint64_t(p.ID)) == nil {
				e.check(C.jh_image_create(e.ctx, C.uint64_t(p.ID), C.uint32_t(p.Width), C.uint32_t(p.Height), C.int(p.Format)), "image_create")
			}
			data := imageData(cmd.Image)
			e.check(C.jh_image_write(e.ctx, C.uint64_t(p.ID), C.uint32_t(cmd.Coords[0]), C.uint32_t(cmd.Coords[1]),
				C.uint32_t(cmd.Coords[2]), C.uint32_t(cmd.Coords[3]), unsafe.Pointer(unsafe.SliceData(data)), C.uint64_t(len(data))), "image_write")
		case *renderer.Dispatch:
			b, pin := e.bind(cmd.Bindings, pendingClears)
			e.check(C.jh_dispatch(e.ctx, C.int(cmd.Shader), C.uint32_t(cmd.WorkgroupSize[0]), C.uint32_t(cmd.WorkgroupSize[1]),
				C.uint32_t(cmd.WorkgroupSize[2]), unsafe.SliceData(b), C.int(len(b))), "dispatch")
			pin.Unpin()
		case *renderer.DispatchIndirect:
			b, pin := e.bind(cmd.Bindings, pendingClears)
			e.check(C.jh_dispatch_indirect(e.ctx, C.int(cmd.Shader), C.uint64_t(cmd.Buffer.ID), C.uint64_t(cmd.Offset),
				unsafe.SliceData(b), C.int(len(b))), "dispatch_indirect")
			pin.Unpin()
		case *renderer.Download: // wgpu.go:554-563, 645-657
			dst := make([]byte, cmd.Buffer.Size)
			e.check(C.jh_download(e.ctx, C.uint64_t(cmd.Buffer.ID), unsafe.Pointer(unsafe.SliceData(dst)), 0,
				C.uint64_t(len(dst))), "download")
			e.downloads[cmd.Buffer.ID] = dst
		case *renderer.Clear:
			if C.jh_buffer_device_ptr(e.ctx, C.uint64_t(cmd.Buffer.ID)) != nil {
				e.check(C.jh_clear(e.ctx, C.uint64_t(cmd.Buffer.ID), C.uint64_t(cmd.Offset), C.int64_t(cmd.Size)), "clear")
			} else {
				pendingClears[cmd.Buffer.ID] = true // wgpu.go:583-585: cleared when the buffer is first bound
			}
		case *renderer.FreeBuffer:
			freeBufs = append(freeBufs, cmd.Buffer.ID)
		case *renderer.FreeImage:
			freeImages = append(freeImages, cmd.Image.ID)
		default:
			panic(fmt.Sprintf("unhandled command %T", cmd))
		}
	}
	for _, id := range freeBufs {
		C.jh_free(e.ctx, C.uint64_t(id))
	}
	for _, id := range freeImages {
		C.jh_image_free(e.ctx, C.uint64_t(id))
	}
}

// The slice is only read during the call: jh_upload copies it into pinned staging memory
// (queue.WriteBuffer semantics, wgpu.go:360).
func (e *Engine) upload(id renderer.ResourceID, data []byte) {
	e.check(C.jh_upload(e.ctx, C.uint64_t(id), unsafe.Pointer(unsafe.SliceData(data)), C.uint64_t(len(data))), "upload")
}

// bind converts []ResourceProxy into []C.jh_binding; transient buffers and images are materialised
// on first use (wgpu.go:877-925).  A runtime.Pinner keeps the image-array id slices alive for the call.
func (e *Engine) bind(res []renderer.ResourceProxy, pendingClears map[renderer.ResourceID]bool) ([]C.jh_binding, *runtime.Pinner) {
	pin := new(runtime.Pinner)
	out := make([]C.jh_binding, len(res))
	for i, r := range res {
		switch r.Kind {
		case renderer.ResourceProxyKindBuffer:
			id := C.uint64_t(r.BufferProxy.ID)
			if C.jh_buffer_device_ptr(e.ctx, id) == nil {
				e.check(C.jh_buffer_create(e.ctx, id, C.uint64_t(r.BufferProxy.Size)), "buffer_create")
				if pendingClears[r.BufferProxy.ID] {
					e.check(C.jh_clear(e.ctx, id, 0, -1), "clear")
					delete(pendingClears, r.BufferProxy.ID)
				}
			}
			out[i] = C.jh_binding{kind: C.JH_BIND_BUFFER, id: id}
		case renderer.ResourceProxyKindImage:
			p := r.ImageProxy
			if C.jh_image_device_ptr(e.ctx, C.uint64_t(p.ID)) == nil {
				e.check(C.jh_image_create(e.ctx, C.uint64_t(p.ID), C.uint32_t(p.Width), C.uint32_t(p.Height), C.int(p.Format)), "image_create")
			}
			out[i] = C.jh_binding{kind: C.JH_BIND_IMAGE, id: C.uint64_t(p.ID)}
		case renderer.ResourceProxyKindImageArray:
			ids := make([]C.uint64_t, len(r.ImageArray))
			for k, p := range r.ImageArray {
				if C.jh_image_device_ptr(e.ctx, C.uint64_t(p.ID)) == nil {
					e.check(C.jh_image_create(e.ctx, C.uint64_t(p.ID), C.uint32_t(p.Width), C.uint32_t(p.Height), C.int(p.Format)), "image_create")
				}
				ids[k] = C.uint64_t(p.ID)
			}
			if len(ids) > 0 {
				pin.Pin(unsafe.SliceData(ids))
			}
			out[i] = C.jh_binding{kind: C.JH_BIND_IMAGE_ARRAY, count: C.uint32_t(len(ids)), ids: unsafe.SliceData(ids)}
		}
	}
	return out, pin
}

// imageData as in wgpu.go:297-320.
func imageData(img image.Image) []byte {
	switch img := img.(type) {
	case *image.NRGBA:
		if img.Stride != 4*img.Rect.Dx() {
			panic("subimages are not supported")
		}
		return img.Pix
	case *image.RGBA:
		if img.Stride != 4*img.Rect.Dx() {
			panic("subimages are not supported")
		}
		return img.Pix
	default:
		panic(fmt.Sprintf("unsupported image type %T", img))
	}
}

// grow is the policy of jello_amd/host/hip_engine.cpp: the reported need plus a quarter.
func grow(have, need uint32) uint32 {
	if need <= have {
		return have
	}
	g := uint64(need) + uint64(need)/4 + 1024
	if g > 0xffffffff {
		g = 0xffffffff
	}
	return uint32(g)
}

// maxClipDepth is the deepest nesting of BeginClip ... EndClip in the encoding's draw tag stream.
func maxClipDepth(enc *encoding.Encoding) uint32 {
	var depth, deepest uint32
	for _, tag := range enc.DrawTags {
		switch tag {
		case encoding.DrawTagBeginClip:
			depth++
			if depth > deepest {
				deepest = depth
			}
		case encoding.DrawTagEndClip:
			if depth > 0 {
				depth--
			}
		}
	}
	return deepest
}

// RenderToTexture mirrors lib.go:244-264 and adds what the fixed sizes of renderer/config.go:141-151
// need for scenes beyond the Vello test scenes: the recording is made with robust = true (it then
// downloads BumpAllocators, render.go:458-460); if bump.Failed is set, the bump-allocated buffers are
// grown to the reported need and the frame is rendered again (Vello's regrow loop).  params.BumpSizes
// (integration/renderer_bump_sizes.patch) carries the sizes; start it from Scene.bumpEstimate
// (scene.go:36-43) -- see DESIGN.md section 1 for the two defects of renderer/estimate.go that make its
// result unusable as it stands -- or from the reference's constants.
// target is device memory for Width*Height RGBA16F pixels.  Returns the attempts it took.
func (e *Engine) RenderToTexture(arena *mem.Arena, enc *encoding.Encoding, target unsafe.Pointer,
	params *renderer.RenderParams, pgroup profiler.ProfilerGroup) int {
	return e.renderToTexture(arena, enc, target, params, pgroup, nil)
}

// renderToTexture is RenderToTexture; outImage, if not nil, receives the target's ImageProxy of the final attempt.
func (e *Engine) renderToTexture(arena *mem.Arena, enc *encoding.Encoding, target unsafe.Pointer,
	params *renderer.RenderParams, pgroup profiler.ProfilerGroup, outImage *renderer.ImageProxy) int {
	for attempt := 1; ; attempt++ {
		var render renderer.Render
		recording := e.renderer.RenderEncodingCoarse(arena, &render, enc, e.resolver, e.fullShaders, params, true, pgroup)
		out := render.OutImage()
		if outImage != nil {
			*outImage = out
		}
		bumpID := render.BumpBuf().ID // (accessor added by the patch; the proxy of the "bumpBuf" buffer)
		recording = e.renderer.RecordFine(arena, &render, e.fullShaders, recording, pgroup)
		// fine's blend-stack scratch is sized from the nesting depth of the clip layers (include/jello_hip.h,
		// jh_set_clip_depth_hint); the hint is taken back after the run so that it never outlives its scene
		// (taken back by a deferred call: a panic inside RunRecording must not leave a stale hint on the context -- a hint
		// that is too small for a later scene loses colours without an error; jh_debug_clip_hint_overflows would tell)
		func() {
			e.check(C.jh_set_clip_depth_hint(e.ctx, C.uint32_t(maxClipDepth(enc))), "set_clip_depth_hint")
			defer C.jh_set_clip_depth_hint(e.ctx, 0)
			e.RunRecording(recording, []ExternalImage{{Proxy: out, DevicePtr: target}}, "RunRecording")
		}()
		raw := e.downloads[bumpID]
		if len(raw) < 32 || attempt >= 6 {
			e.check(C.jh_sync(e.ctx), "sync")
			return attempt
		}
		var b renderer.BumpAllocators // Failed Binning Ptcl Tile SegCounts Segments Blend Lines (config.go:301-312)
		b.Failed = binary.LittleEndian.Uint32(raw[0:])
		b.Binning = binary.LittleEndian.Uint32(raw[4:])
		b.Ptcl = binary.LittleEndian.Uint32(raw[8:])
		b.Tile = binary.LittleEndian.Uint32(raw[12:])
		b.SegCounts = binary.LittleEndian.Uint32(raw[16:])
		b.Segments = binary.LittleEndian.Uint32(raw[20:])
		b.Blend = binary.LittleEndian.Uint32(raw[24:])
		b.Lines = binary.LittleEndian.Uint32(raw[28:])
		if b.Failed == 0 {
			e.check(C.jh_sync(e.ctx), "sync")
			return attempt
		}
		s := params.BumpSizes
		before := *s
		widthInTiles, heightInTiles := (params.Width+15)/16, (params.Height+15)/16
		s.Lines = grow(s.Lines, b.Lines)
		s.BinData = grow(s.BinData, b.Binning+render.Layout().BinDataStart)
		s.Tiles = grow(s.Tiles, b.Tile)
		s.SegCounts = grow(s.SegCounts, b.SegCounts)
		s.Segments = grow(s.Segments, max(b.Segments, b.SegCounts))
		s.BlendSpill = grow(s.BlendSpill, b.Blend)
		s.Ptcl = grow(s.Ptcl, b.Ptcl+widthInTiles*heightInTiles*64)
		if before == *s {
			return attempt // nothing left to grow
		}
	}
}

// RenderToSurface mirrors lib.go:266-333: RenderToTexture into the engine's own RGBA16F target (kept while the size stays
// the same, lib.go:279-284), then the blit pass (lib.go:109-198) -- premultiply, convert to format -- into surface: device
// memory of params.Height rows of 4*params.Width bytes, pitch bytes apart (bytes past 4*Width are not written).  The blit is
// stream-ordered behind the frame; the surface is ready once the context's stream is (the regrow loop of RenderToTexture
// already waited for the frame).  Returns the attempts RenderToTexture took.
func (e *Engine) RenderToSurface(arena *mem.Arena, enc *encoding.Encoding, surface unsafe.Pointer, pitch uint64,
	format SurfaceFormat, params *renderer.RenderParams, pgroup profiler.ProfilerGroup) int {
	label := C.CString("RenderToSurface")
	defer C.free(unsafe.Pointer(label))
	e.check(C.jh_profile_group_begin(e.ctx, label), "profile_group_begin")
	defer C.jh_profile_group_end(e.ctx)
	if e.target == nil || e.target.Width != params.Width || e.target.Height != params.Height {
		if e.target != nil {
			e.check(C.jh_free(e.ctx, C.uint64_t(e.target.id)), "free")
		}
		id := surfaceTargetID
		e.check(C.jh_buffer_create(e.ctx, C.uint64_t(id), C.uint64_t(uint64(params.Width)*uint64(params.Height)*8)), "buffer_create")
		e.target = &targetTexture{id: id, ptr: C.jh_buffer_device_ptr(e.ctx, C.uint64_t(id)), Width: params.Width, Height: params.Height}
	}
	var out renderer.ImageProxy
	attempts := e.renderToTexture(arena, enc, e.target.ptr, params, pgroup, &out)
	e.check(C.jh_blit(e.ctx, C.uint64_t(out.ID), surface, C.uint64_t(pitch), C.uint32_t(params.Width), C.uint32_t(params.Height),
		C.int(format)), "blit")
	// the target image of this frame is an import over e.target: forgetting it frees nothing
	e.check(C.jh_image_free(e.ctx, C.uint64_t(out.ID)), "image_free")
	return attempts
}

// RenderToYUV is RenderToSurface for a video encoder: RenderToTexture into the same engine-owned RGBA16F target, then
// jh_blit_yuv into planar 8-bit Y'CbCr 4:2:0 -- planes[0] = Y, planes[1] = interleaved CbCr (NV12) or Cb (I420), planes[2] = Cr
// (I420 only; YV12 is I420 with the two chroma pointers swapped) -- device memory with pitches[i] bytes between rows.  Bytes past
// a row's end and rows below a plane are not written.  Stream-ordered behind the frame.  Returns the attempts
// RenderToTexture took.
func (e *Engine) RenderToYUV(arena *mem.Arena, enc *encoding.Encoding, planes [3]unsafe.Pointer, pitches [3]uint64, format YUVFormat,
	params *renderer.RenderParams, pgroup profiler.ProfilerGroup) int {
	label := C.CString("RenderToYUV")
	defer C.free(unsafe.Pointer(label))
	e.check(C.jh_profile_group_begin(e.ctx, label), "profile_group_begin")
	defer C.jh_profile_group_end(e.ctx)
	if e.target == nil || e.target.Width != params.Width || e.target.Height != params.Height {
		if e.target != nil {
			e.check(C.jh_free(e.ctx, C.uint64_t(e.target.id)), "free")
		}
		id := surfaceTargetID
		e.check(C.jh_buffer_create(e.ctx, C.uint64_t(id), C.uint64_t(uint64(params.Width)*uint64(params.Height)*8)), "buffer_create")
		e.target = &targetTexture{id: id, ptr: C.jh_buffer_device_ptr(e.ctx, C.uint64_t(id)), Width: params.Width, Height: params.Height}
	}
	var out renderer.ImageProxy
	attempts := e.renderToTexture(arena, enc, e.target.ptr, params, pgroup, &out)
	var d C.jh_yuv_desc
	d.layout, d.matrix = C.int32_t(format.Layout), C.int32_t(format.Matrix)
	d._range, d.transfer = C.int32_t(format.Range), C.int32_t(format.Transfer) // (cgo spells the C field `range` _range)
	for i := range planes {
		d.plane[i] = planes[i]
		d.pitch[i] = C.uint64_t(pitches[i])
	}
	e.check(C.jh_blit_yuv(e.ctx, C.uint64_t(out.ID), C.uint32_t(params.Width), C.uint32_t(params.Height), &d), "blit_yuv")
	// the target image of this frame is an import over e.target: forgetting it frees nothing
	e.check(C.jh_image_free(e.ctx, C.uint64_t(out.ID)), "image_free")
	return attempts
}

// packBufferID names the pack's memory on the context for the two downloads of ReadPack (see surfaceTargetID).
const packBufferID renderer.ResourceID = 1<<63 | 0x7061636b00000000

// PackBound is jh_pack_bound: the size of the largest pack of a width x height frame (0 for a texel size other than 4 or 8).
func PackBound(width, height, texelBytes uint32) uint64 {
	return uint64(C.jh_pack_bound(C.uint32_t(width), C.uint32_t(height), C.uint32_t(texelBytes)))
}

// PackTiles is jh_pack_tiles (the format: include/jello_hip.h): the frame at src -- a surface RenderToSurface wrote
// (texelBytes 4) or an RGBA16F target (8), rows srcPitch bytes apart -- as a tile pack in dst (capacity >= PackBound), against
// the reference frame at ref unless that is nil.  Device memory throughout; stream-ordered, waits for nothing.
func (e *Engine) PackTiles(src unsafe.Pointer, srcPitch uint64, ref unsafe.Pointer, refPitch uint64, width, height, texelBytes uint32,
	dst unsafe.Pointer, capacity uint64) {
	e.check(C.jh_pack_tiles(e.ctx, src, C.uint64_t(srcPitch), ref, C.uint64_t(refPitch), C.uint32_t(width), C.uint32_t(height),
		C.uint32_t(texelBytes), dst, C.uint64_t(capacity)), "pack_tiles")
}

// DashEl, DashPath are jh_dash_el and jh_dash_path (include/jello_hip.h "dashing").
type DashEl struct {
	Kind, _ int32
	Pts     [6]float64
}
type DashPath struct {
	FirstEl, NEls, FirstDash, NDash uint32
	Offset                          float64
}

// DashPaths is jh_dash: the dashes of a batch of paths by the rule of DESIGN.md 5.6, computed on the device.  els, paths and
// dashes are host slices read during the call; outEls (capacity elements of 28 bytes) and outIndex (len(paths)+1 words) are
// device memory.  Stream-ordered, waits for nothing: the last index word reports the elements the job needs -- regrow and call
// again when it exceeds capacity.  The Go Scene keeps curve.Dash (scene.go:169-177); this is the opt-in device route for callers
// that dash many paths.
func (e *Engine) DashPaths(els []DashEl, paths []DashPath, dashes []float64, outEls unsafe.Pointer, capacity uint64, outIndex unsafe.Pointer) {
	var pe *C.jh_dash_el
	var pp *C.jh_dash_path
	var pd *C.double
	if len(els) > 0 {
		pe = (*C.jh_dash_el)(unsafe.Pointer(&els[0]))
	}
	if len(paths) > 0 {
		pp = (*C.jh_dash_path)(unsafe.Pointer(&paths[0]))
	}
	if len(dashes) > 0 {
		pd = (*C.double)(unsafe.Pointer(&dashes[0]))
	}
	e.check(C.jh_dash(e.ctx, pe, C.uint64_t(len(els)), pp, C.uint32_t(len(paths)), pd, C.uint64_t(len(dashes)), outEls,
		C.uint64_t(capacity), (*C.uint32_t)(outIndex)), "dash")
}

// BlurEdge is jh_blur_edge: what a tap outside the image reads.
type BlurEdge int32

const (
	BlurEdgeZero  BlurEdge = 0 // nothing
	BlurEdgeClamp BlurEdge = 1 // the nearest texel of the image
)

// BlurDesc is jh_blur_desc (include/jello_hip.h "Gaussian blur"): the standard deviations of the two axes (0 .. 64), the edge
// mode and the rectangle of dst that is written (Width == Height == 0: the whole image).
type BlurDesc struct {
	SigmaX, SigmaY      float32
	Edge                BlurEdge
	X, Y, Width, Height uint32
}

// Blur is jh_blur: the Gaussian blur of the RGBA16F image src into the rectangle of dst that desc names, by the rule of
// DESIGN.md 5.7 (defined on values: every implementation gives the same bits).  dst may be src.  Texels of dst outside the
// rectangle keep their bits; source texels outside it take part.  Stream-ordered behind the frame, waits for nothing; for drop
// shadows, glows, backdrop blur, feGaussianBlur and CSS blur() between RenderToTexture and the surface / YUV / pack conversion.
func (e *Engine) Blur(src, dst renderer.ImageProxy, desc BlurDesc) {
	d := C.jh_blur_desc{sigma_x: C.float(desc.SigmaX), sigma_y: C.float(desc.SigmaY), edge: C.int(desc.Edge), x: C.uint32_t(desc.X),
		y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height)}
	e.check(C.jh_blur(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), C.uint32_t(src.Width), C.uint32_t(src.Height), &d), "blur")
}

// CompositeTint is JH_COMPOSITE_TINT: the source's colour is replaced by CompositeDesc.Tint's and its alpha scaled by Tint[3].
const CompositeTint uint32 = 1

// CompositeDesc is jh_composite_desc (include/jello_hip.h "Composite"): the mix mode (0..15, not Clip) and the Porter-Duff operator
// (0..13) in the encodings of gfx, an opacity in [0, 1], the flags, the tint (read only with CompositeTint), the rectangle of the
// source that is placed (SW == SH == 0: the whole source) and where its top-left lands in dst (clipped to dst).
type CompositeDesc struct {
	Mix, Compose   uint32
	Opacity        float32
	Flags          uint32
	Tint           [4]float32
	SX, SY, SW, SH uint32
	DX, DY         int32
}

// Composite is jh_composite: the RGBA16F image src blended onto the RGBA16F image dst (another image; the sizes may differ) by the
// rule of DESIGN.md 5.8 (defined on values: every implementation gives the same bits) -- the blend the fine stage applies to a
// layer, image to image.  Only the placed rectangle is written.  Stream-ordered behind the frame, waits for nothing, one kernel
// launch; with Blur it makes a drop shadow: blur the layer into a scratch image, Composite that with a tint and an offset, Composite
// the layer.
func (e *Engine) Composite(src, dst renderer.ImageProxy, desc CompositeDesc) {
	d := C.jh_composite_desc{mix: C.uint32_t(desc.Mix), compose: C.uint32_t(desc.Compose), opacity: C.float(desc.Opacity), flags: C.uint32_t(desc.Flags),
		sx: C.uint32_t(desc.SX), sy: C.uint32_t(desc.SY), sw: C.uint32_t(desc.SW), sh: C.uint32_t(desc.SH), dx: C.int32_t(desc.DX), dy: C.int32_t(desc.DY)}
	for i, v := range desc.Tint {
		d.tint[i] = C.float(v)
	}
	e.check(C.jh_composite(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "composite")
}

// ResampleFilter is jh_resample_filter: the kernel of Resample, by its support at 1:1.
type ResampleFilter int32

const (
	ResampleBox        ResampleFilter = 0 // 0.5 texels
	ResampleTriangle   ResampleFilter = 1 // 1
	ResampleCatmullRom ResampleFilter = 2 // 2
	ResampleLanczos3   ResampleFilter = 3 // 3
)

// ResampleStraight is JH_RESAMPLE_STRAIGHT: the four channels are filtered as they are stored, colour is not weighted by alpha.
const ResampleStraight uint32 = 1

// ResampleDesc is jh_resample_desc (include/jello_hip.h "Resample"): the filter, the flags, and the rectangles of the source that is
// read and of the destination that is written (Width == Height == 0: the whole image).
type ResampleDesc struct {
	Filter                          ResampleFilter
	Flags                           uint32
	SrcX, SrcY, SrcWidth, SrcHeight uint32
	DstX, DstY, DstWidth, DstHeight uint32
}

// Resample is jh_resample: a rectangle of the RGBA16F image src resized into a rectangle of the RGBA16F image dst (another image)
// by the rule of DESIGN.md 5.9 (defined on values: every implementation gives the same bits), at most 16:1 down on either axis.
// Only the destination rectangle is written.  Stream-ordered behind the frame, waits for nothing, two kernel launches; the context
// keeps the tap tables of one geometry (filter and the rectangles' extents), so a call that repeats the last one's uploads nothing
// and can be captured.  For a video frame or a thumbnail of a larger render, a supersampled render at display size, mip levels, a
// layer scaled before Composite places it.
func (e *Engine) Resample(src, dst renderer.ImageProxy, desc ResampleDesc) {
	d := C.jh_resample_desc{filter: C.int(desc.Filter), flags: C.uint32_t(desc.Flags), src_x: C.uint32_t(desc.SrcX), src_y: C.uint32_t(desc.SrcY),
		src_width: C.uint32_t(desc.SrcWidth), src_height: C.uint32_t(desc.SrcHeight), dst_x: C.uint32_t(desc.DstX), dst_y: C.uint32_t(desc.DstY),
		dst_width: C.uint32_t(desc.DstWidth), dst_height: C.uint32_t(desc.DstHeight)}
	e.check(C.jh_resample(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "resample")
}

// ColorSpace is jh_color_space: the values the matrix and the funcs of ColorFilter act on.
type ColorSpace int32

const (
	ColorLinear ColorSpace = 0 // the stored, linear values
	ColorSRGB   ColorSpace = 1 // colour channels sRGB-encoded before the matrix and decoded after the funcs; alpha never
)

// ColorFuncType is jh_color_func_type: feComponentTransfer's function types.
type ColorFuncType int32

const (
	ColorFuncIdentity ColorFuncType = 0
	ColorFuncLinear   ColorFuncType = 1 // Slope, Intercept
	ColorFuncGamma    ColorFuncType = 2 // Amplitude, Exponent, Offset
	ColorFuncTable    ColorFuncType = 3 // Values, 1..64 of them
	ColorFuncDiscrete ColorFuncType = 4 // Values, 1..64 of them
)

// ColorClamp is JH_COLOR_CLAMP: the matrix's result and each func's are clamped to [0, 1].
const ColorClamp uint32 = 1

// ColorFunc is jh_color_func: the transfer function of one output channel.
type ColorFunc struct {
	Type                        ColorFuncType
	Slope, Intercept            float32
	Amplitude, Exponent, Offset float32
	Values                      []float32
}

// ColorDesc is jh_color_desc (include/jello_hip.h "Colour filter"): the rectangle, in both images (Width == Height == 0: the whole
// image), the row-major 4 x 5 matrix on the un-premultiplied (r, g, b, a, 1), the space, the flags and the four funcs.
type ColorDesc struct {
	X, Y, Width, Height uint32
	Matrix              [20]float32
	Space               ColorSpace
	Flags               uint32
	Func                [4]ColorFunc
}

// ColorFilter is jh_color_filter: a colour matrix and per-channel transfer functions on a rectangle of the RGBA16F image src,
// written to the same rectangle of the RGBA16F image dst (which may be src) by the rule of DESIGN.md 5.10 (defined on values: every
// implementation gives the same bits).  feColorMatrix, feComponentTransfer, the CSS filter functions, a tint, the first half of a
// luminance mask.  Stream-ordered behind the frame, waits for nothing, one kernel launch; the context keeps the tables of one key
// (space, clamp bit, funcs), so a call that repeats the last one's uploads nothing and can be captured; LINEAR space with IDENTITY
// funcs needs no tables.  More than 64 values in a func are the call's to refuse.
func (e *Engine) ColorFilter(src, dst renderer.ImageProxy, desc ColorDesc) {
	d := C.jh_color_desc{x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height),
		space: C.int(desc.Space), flags: C.uint32_t(desc.Flags)}
	for i, m := range desc.Matrix {
		d.matrix[i] = C.float(m)
	}
	for i, f := range desc.Func {
		c := &d._func[i]
		c._type = C.int(f.Type)
		c.n = C.uint32_t(len(f.Values))
		c.slope, c.intercept = C.float(f.Slope), C.float(f.Intercept)
		c.amplitude, c.exponent, c.offset = C.float(f.Amplitude), C.float(f.Exponent), C.float(f.Offset)
		for k, v := range f.Values {
			if k < len(c.values) {
				c.values[k] = C.float(v)
			}
		}
	}
	e.check(C.jh_color_filter(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "color_filter")
}

// MorphOp is jh_morph_op: the least (erode) or the greatest (dilate) operand of the window.
type MorphOp int32

const (
	MorphErode  MorphOp = 0
	MorphDilate MorphOp = 1
)

// MorphEdge is jh_morph_edge: what a position outside the image is.
type MorphEdge int32

const (
	MorphEdgeZero  MorphEdge = 0 // transparent black takes part (feMorphology)
	MorphEdgeClamp MorphEdge = 1 // the position does not take part
)

// MorphStraight is JH_MORPH_STRAIGHT: the operands are the four channels as stored, not colour times alpha.
const MorphStraight uint32 = 1

// MorphDesc is jh_morph_desc (include/jello_hip.h "Morphology"): the operator, the edge mode, the flags, the radii (0..255 each) and
// the rectangle of dst that is written (Width == Height == 0: the whole image).
type MorphDesc struct {
	Op                  MorphOp
	Edge                MorphEdge
	Flags               uint32
	RadiusX, RadiusY    uint32
	X, Y, Width, Height uint32
}

// Morphology is jh_morphology: the RGBA16F image src eroded or dilated by a box of (2 RadiusX + 1) x (2 RadiusY + 1) texels into the
// rectangle of the RGBA16F image dst of the same size (which may be src) by the rule of DESIGN.md 5.11 (defined on values: every
// implementation gives the same bits).  A shadow's spread, an outline, a choked matte, feMorphology.  Stream-ordered behind the frame,
// waits for nothing, three kernel launches whatever the radius; the intermediate lives in a scratch array of the context that only
// grows, so a call can be captured once one of its rectangle size and radii has run eagerly.
func (e *Engine) Morphology(src, dst renderer.ImageProxy, desc MorphDesc) {
	d := C.jh_morph_desc{op: C.int(desc.Op), edge: C.int(desc.Edge), flags: C.uint32_t(desc.Flags), radius_x: C.uint32_t(desc.RadiusX),
		radius_y: C.uint32_t(desc.RadiusY), x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height)}
	e.check(C.jh_morphology(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "morphology")
}

// WarpFilter is jh_warp_filter: 1, 2 x 2 or 4 x 4 (Catmull-Rom) source texels per destination texel.
type WarpFilter int32

const (
	WarpNearest  WarpFilter = 0
	WarpBilinear WarpFilter = 1
	WarpBicubic  WarpFilter = 2
)

// WarpEdge is jh_warp_edge: what a tap outside the source rectangle reads.
type WarpEdge int32

const (
	WarpEdgeZero   WarpEdge = 0 // transparent black
	WarpEdgeClamp  WarpEdge = 1 // the nearest texel of the rectangle
	WarpEdgeRepeat WarpEdge = 2 // the rectangle tiled (feTile)
	WarpEdgeMirror WarpEdge = 3 // the rectangle tiled, every other copy flipped
)

// WarpStraight is JH_WARP_STRAIGHT: the four channels are filtered as stored, not colour times alpha.
const WarpStraight uint32 = 1

// WarpDesc is jh_warp_desc (include/jello_hip.h "Warp"): the matrix (a, b, c, d, e, f) in the order the Scene transforms use, from
// continuous coordinates of the source rectangle to continuous coordinates of the destination IMAGE, the filter, the edge mode, the
// flags, and the two rectangles (Width == Height == 0: the whole image); the destination rectangle is only what gets written.
type WarpDesc struct {
	Matrix                          [6]float64
	Filter                          WarpFilter
	Edge                            WarpEdge
	Flags                           uint32
	SrcX, SrcY, SrcWidth, SrcHeight uint32
	DstX, DstY, DstWidth, DstHeight uint32
}

// Warp is jh_warp: a rectangle of the RGBA16F image src under an affine map into a rectangle of the RGBA16F image dst (another image)
// by the rule of DESIGN.md 5.12 (defined on values: every implementation gives the same bits).  A rotated, skewed or
// sub-texel-translated layer, a CSS transform on a filtered layer, a tiled pattern under WarpEdgeRepeat.  No minification prefilter:
// below about 1:2 Resample comes first.  Stream-ordered behind the frame, waits for nothing, one kernel launch, no scratch and no
// tables: always capturable.
func (e *Engine) Warp(src, dst renderer.ImageProxy, desc WarpDesc) {
	d := C.jh_warp_desc{filter: C.int(desc.Filter), edge: C.int(desc.Edge), flags: C.uint32_t(desc.Flags),
		src_x: C.uint32_t(desc.SrcX), src_y: C.uint32_t(desc.SrcY), src_width: C.uint32_t(desc.SrcWidth), src_height: C.uint32_t(desc.SrcHeight),
		dst_x: C.uint32_t(desc.DstX), dst_y: C.uint32_t(desc.DstY), dst_width: C.uint32_t(desc.DstWidth), dst_height: C.uint32_t(desc.DstHeight)}
	for i, m := range desc.Matrix {
		d.matrix[i] = C.double(m)
	}
	e.check(C.jh_warp(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "warp")
}

// ConvolveEdge is jh_convolve_edge: what a tap outside the image reads (WarpEdge's values: feConvolveMatrix's edgeMode none,
// duplicate and wrap, and the image mirrored).
type ConvolveEdge int32

const (
	ConvolveEdgeZero   ConvolveEdge = 0
	ConvolveEdgeClamp  ConvolveEdge = 1
	ConvolveEdgeRepeat ConvolveEdge = 2
	ConvolveEdgeMirror ConvolveEdge = 3
)

// ConvolveMode is jh_convolve_mode: the operand -- colour times alpha, the four channels as stored, or the colour channels as stored
// with the source's alpha copied (preserveAlpha).
type ConvolveMode int32

const (
	ConvolvePremultiplied ConvolveMode = 0
	ConvolveStraight      ConvolveMode = 1
	ConvolvePreserveAlpha ConvolveMode = 2
)

// ConvolveDesc is jh_convolve_desc (include/jello_hip.h "Convolve"): the orders (1..15), the target, the edge mode, the operand mode,
// the bias, the rectangle of dst that is written (Width == Height == 0: the whole image) and the weights, row-major with stride
// OrderX, IN THE ORDER THEY ARE APPLIED (ConvolveWeights makes them of feConvolveMatrix's kernelMatrix and divisor).
type ConvolveDesc struct {
	OrderX, OrderY, TargetX, TargetY uint32
	Edge                             ConvolveEdge
	Mode                             ConvolveMode
	Bias                             float32
	X, Y, Width, Height              uint32
	Weights                          []float32
}

// ConvolveWeights is jh_convolve_weights: feConvolveMatrix's kernelMatrix (orderX * orderY values, row-major) rotated by 180 degrees
// and divided by divisor (0: the sum of the matrix, or 1 if that is 0), in binary64, rounded once to binary32.  Host only.
func ConvolveWeights(orderX, orderY uint32, kernelMatrix []float64, divisor float64) ([]float32, error) {
	if orderX < 1 || orderX > 15 || orderY < 1 || orderY > 15 || uint32(len(kernelMatrix)) != orderX*orderY {
		return nil, fmt.Errorf("hip_engine: ConvolveWeights: an order outside 1..15, or a kernelMatrix of another length")
	}
	w := make([]float32, orderX*orderY)
	if C.jh_convolve_weights(C.uint32_t(orderX), C.uint32_t(orderY), (*C.double)(unsafe.Pointer(&kernelMatrix[0])), C.double(divisor), (*C.float)(unsafe.Pointer(&w[0]))) != 0 {
		return nil, fmt.Errorf("hip_engine: ConvolveWeights: a non-finite input, or a weight that does not come out finite")
	}
	return w, nil
}

// Convolve is jh_convolve: the RGBA16F image src under a small convolution kernel into the RGBA16F image dst (another image of the
// same size) by the rule of DESIGN.md 5.13 (defined on values: every implementation gives the same bits) -- sharpen, emboss, edge
// detection, any kernel up to 15 x 15.  Stream-ordered behind the frame, waits for nothing, one kernel launch, no scratch and no
// tables: always capturable.
func (e *Engine) Convolve(src, dst renderer.ImageProxy, desc ConvolveDesc) {
	d := C.jh_convolve_desc{order_x: C.uint32_t(desc.OrderX), order_y: C.uint32_t(desc.OrderY), target_x: C.uint32_t(desc.TargetX),
		target_y: C.uint32_t(desc.TargetY), edge: C.int(desc.Edge), mode: C.int(desc.Mode), bias: C.float(desc.Bias),
		x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height)}
	for i, w := range desc.Weights {
		if i < len(d.weights) {
			d.weights[i] = C.float(w)
		}
	}
	e.check(C.jh_convolve(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "convolve")
}

// LightKind is jh_lighting_kind: feDiffuseLighting or feSpecularLighting.
type LightKind int32

const (
	LightingDiffuse  LightKind = 0
	LightingSpecular LightKind = 1
)

// LightSource is jh_light_source: feDistantLight, fePointLight, feSpotLight.
type LightSource int32

const (
	LightDistant LightSource = 0
	LightPoint   LightSource = 1
	LightSpot    LightSource = 2
)

// LightingDesc is jh_lighting_desc (include/jello_hip.h "Lighting"): the filter (SurfaceScale, Constant = kd or ks, SpecularExponent in
// [1, 128], a LINEAR Color), the light (Direction towards a distant light; Position of a point or spot light, PointsAt, SpotExponent in
// [1, 128] and ConeCos, the cosine of the limiting cone angle, -1: no cone) in texels of the image, texel (X, Y) at (X + 0.5, Y + 0.5),
// and the rectangle of dst that is written (Width == Height == 0: the whole image).
type LightingDesc struct {
	Kind                                                  LightKind
	Light                                                 LightSource
	SurfaceScale, Constant, SpecularExponent, SpotExponent float32
	Color                                                 [3]float32
	X, Y, Width, Height                                   uint32
	Direction, Position, PointsAt                         [3]float64
	ConeCos                                               float64
}

// LightPlan is jh_light_plan: what the device is given of a LightingDesc, every value a binary32.
type LightPlan struct {
	S                [2][3]float32 // [span - 1][wsum - 2]
	Ldir, P, Sdir    [3]float32
	Cone             float32
}

func (desc LightingDesc) c() C.jh_lighting_desc {
	d := C.jh_lighting_desc{kind: C.int(desc.Kind), light: C.int(desc.Light), surface_scale: C.float(desc.SurfaceScale), constant: C.float(desc.Constant),
		specular_exponent: C.float(desc.SpecularExponent), spot_exponent: C.float(desc.SpotExponent), x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y),
		width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height), cone_cos: C.double(desc.ConeCos)}
	for i := 0; i < 3; i++ {
		d.color[i] = C.float(desc.Color[i])
		d.direction[i] = C.double(desc.Direction[i])
		d.position[i] = C.double(desc.Position[i])
		d.points_at[i] = C.double(desc.PointsAt[i])
	}
	return d
}

// LightingPlan is jh_lighting_plan: the plan of desc -- the only place binary64 appears in the lighting rule.  Host only.
func LightingPlan(desc LightingDesc) (LightPlan, error) {
	d := desc.c()
	var p C.jh_light_plan
	if C.jh_lighting_plan(&d, &p) != 0 {
		return LightPlan{}, fmt.Errorf("hip_engine: LightingPlan: a descriptor the rule refuses")
	}
	var out LightPlan
	for i := 0; i < 2; i++ {
		for j := 0; j < 3; j++ {
			out.S[i][j] = float32(p.s[i][j])
		}
	}
	for i := 0; i < 3; i++ {
		out.Ldir[i], out.P[i], out.Sdir[i] = float32(p.ldir[i]), float32(p.p[i]), float32(p.sdir[i])
	}
	out.Cone = float32(p.cone)
	return out, nil
}

// Lighting is jh_lighting: feDiffuseLighting or feSpecularLighting of the ALPHA channel of the RGBA16F image src into the RGBA16F
// image dst (another image of the same size) by the rule of DESIGN.md 5.14 (defined on values: every implementation gives the same
// bits).  Stream-ordered behind the frame, waits for nothing, one kernel launch.  The context holds the power tables of one pair of
// exponents: a call with another uploads its own and makes graphs captured before it stale; exponents of 1 need none.
func (e *Engine) Lighting(src, dst renderer.ImageProxy, desc LightingDesc) {
	d := desc.c()
	e.check(C.jh_lighting(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "lighting")
}

// TurbulenceKind is jh_turbulence_kind: feTurbulence's type.
type TurbulenceKind int32

const (
	TurbulenceFractalNoise TurbulenceKind = 0
	TurbulenceTurbulence   TurbulenceKind = 1
)

// TurbulenceDesc is jh_turbulence_desc (include/jello_hip.h "Turbulence"): the kind, BaseFrequency in cells per texel (>= 0), Octaves
// 0 .. 16, the Seed, Stitch with its Tile (x, y, w, h; read only under Stitch), Origin: the coordinate of the image's corner -- texel
// (X, Y) is the noise at (Origin[0] + X + 0.5, Origin[1] + Y + 0.5) --, and the rectangle of dst that is written (Width == Height ==
// 0: the whole image).
type TurbulenceDesc struct {
	Kind                TurbulenceKind
	Octaves             uint32
	Seed                int32
	Stitch              bool
	X, Y, Width, Height uint32
	BaseFrequency       [2]float64
	Tile                [4]float64
	Origin              [2]float64
}

// TurbPlan is jh_turb_plan: what the device is given of a TurbulenceDesc -- the frequency after the stitch adjustment, the int64
// positions in units of 2^-32 cell, the stitch pair, the largest legal image extent and the key of the tables.
type TurbPlan struct {
	Frequency   [2]float64
	Step, Start [2]int64
	Wrap, Width [2]int32
	MaxExtent   [2]uint32
	Key         uint32
	Stitched    bool
}

func (desc TurbulenceDesc) c() C.jh_turbulence_desc {
	d := C.jh_turbulence_desc{kind: C.int(desc.Kind), octaves: C.uint32_t(desc.Octaves), seed: C.int32_t(desc.Seed), x: C.uint32_t(desc.X),
		y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height)}
	if desc.Stitch {
		d.stitch = 1
	}
	for i := 0; i < 2; i++ {
		d.base_frequency[i] = C.double(desc.BaseFrequency[i])
		d.origin[i] = C.double(desc.Origin[i])
	}
	for i := 0; i < 4; i++ {
		d.tile[i] = C.double(desc.Tile[i])
	}
	return d
}

// TurbulencePlan is jh_turbulence_plan: the plan of desc -- with the tables the only place binary64 appears in the turbulence rule.
// Host only.
func TurbulencePlan(desc TurbulenceDesc) (TurbPlan, error) {
	d := desc.c()
	var p C.jh_turb_plan
	if C.jh_turbulence_plan(&d, &p) != 0 {
		return TurbPlan{}, fmt.Errorf("hip_engine: TurbulencePlan: a descriptor the rule refuses")
	}
	var out TurbPlan
	for i := 0; i < 2; i++ {
		out.Frequency[i], out.Step[i], out.Start[i] = float64(p.frequency[i]), int64(p.step[i]), int64(p.start[i])
		out.Wrap[i], out.Width[i], out.MaxExtent[i] = int32(p.wrap[i]), int32(p.width[i]), uint32(p.max_extent[i])
	}
	out.Key, out.Stitched = uint32(p.key), p.stitched != 0
	return out, nil
}

// Turbulence is jh_turbulence: feTurbulence -- Perlin turbulence or fractal noise, all four channels, straight colour -- GENERATED into
// the RGBA16F image dst by the rule of DESIGN.md 5.15 (defined on values: every implementation gives the same bits).  Stream-ordered
// behind the frame, waits for nothing, one kernel launch.  The context holds the tables of one seed: a call with another uploads its
// own (8.4 KB) and makes graphs captured before it stale.
func (e *Engine) Turbulence(dst renderer.ImageProxy, desc TurbulenceDesc) {
	d := desc.c()
	e.check(C.jh_turbulence(e.ctx, C.uint64_t(dst.ID), &d), "turbulence")
}

// DisplaceChannel is jh_displace_channel: the channel of the map that moves an axis (feDisplacementMap's xChannelSelector and
// yChannelSelector).
type DisplaceChannel int32

const (
	DisplaceR DisplaceChannel = 0
	DisplaceG DisplaceChannel = 1
	DisplaceB DisplaceChannel = 2
	DisplaceA DisplaceChannel = 3
)

// DisplaceStraight is JH_DISPLACE_STRAIGHT: the source's four channels are filtered as stored, not colour times alpha.
const DisplaceStraight uint32 = 1

// DisplaceDesc is jh_displace_desc (include/jello_hip.h "Displace"): WarpDesc's fields with WarpDesc's meaning -- the identity matrix
// is what feDisplacementMap needs -- then the scales, in texels of the source rectangle per unit of map value, and the two channels.
type DisplaceDesc struct {
	Matrix                          [6]float64
	Filter                          WarpFilter
	Edge                            WarpEdge
	Flags                           uint32
	SrcX, SrcY, SrcWidth, SrcHeight uint32
	DstX, DstY, DstWidth, DstHeight uint32
	ScaleX, ScaleY                  float32
	XChannel, YChannel              DisplaceChannel
}

// DisplaceOffset is jh_displace_offset: the displacement, in units of 2^-32 texel, that the map value with the f16 bit pattern bits
// gives under scale -- rint(clamp(scale (m - 0.5), +-2^22) 2^32), a NaN product counting as 0 (DESIGN.md 5.17).  No context, no device.
func DisplaceOffset(scale float32, bits uint16) int64 {
	var out C.int64_t
	C.jh_displace_offset(C.float(scale), C.uint16_t(bits), &out)
	return int64(out)
}

// Displace is jh_displace: feDisplacementMap -- Warp of src into dst (another image) with every destination texel's source position
// moved by scale x (m - 0.5), m the chosen channels of the texel at the same place of the RGBA16F image dmap, which has dst's size and
// is read as stored -- by the rule of DESIGN.md 5.17 (defined on values: every implementation gives the same bits).  dmap may be dst
// (noise generated into dst by Turbulence and displaced over in place) or src.  Stream-ordered behind the frame, waits for nothing,
// one kernel launch, no scratch and no tables: always capturable.
func (e *Engine) Displace(src, dmap, dst renderer.ImageProxy, desc DisplaceDesc) {
	d := C.jh_displace_desc{filter: C.int(desc.Filter), edge: C.int(desc.Edge), flags: C.uint32_t(desc.Flags),
		src_x: C.uint32_t(desc.SrcX), src_y: C.uint32_t(desc.SrcY), src_width: C.uint32_t(desc.SrcWidth), src_height: C.uint32_t(desc.SrcHeight),
		dst_x: C.uint32_t(desc.DstX), dst_y: C.uint32_t(desc.DstY), dst_width: C.uint32_t(desc.DstWidth), dst_height: C.uint32_t(desc.DstHeight),
		scale_x: C.float(desc.ScaleX), scale_y: C.float(desc.ScaleY), x_channel: C.int(desc.XChannel), y_channel: C.int(desc.YChannel)}
	for i, m := range desc.Matrix {
		d.matrix[i] = C.double(m)
	}
	e.check(C.jh_displace(e.ctx, C.uint64_t(src.ID), C.uint64_t(dmap.ID), C.uint64_t(dst.ID), &d), "displace")
}

// ShadowOver and ShadowInvert are JH_SHADOW_OVER and JH_SHADOW_INVERT: the shadow is laid over what dst holds (Normal + SrcOver, in
// place); the coverage is 1 - S (inset shadows).
const (
	ShadowOver   uint32 = 1
	ShadowInvert uint32 = 2
)

// ShadowDesc is jh_shadow_desc (include/jello_hip.h "Shadow"): Matrix takes shape space to dst's texel space, the rectangle of dst
// that is written (Width == Height == 0: the whole image), the flags, Radius and Sigma in shape units, Box = x0, y0, x1, y1 in shape
// space and Color, premultiplied and linear.
type ShadowDesc struct {
	Matrix              [6]float64
	X, Y, Width, Height uint32
	Flags               uint32
	Radius, Sigma       float32
	Box                 [4]float32
	Color               [4]float32
}

// ShadPlan is jh_shad_plan: the six integers of the matrix, the box's centre in units of 2^-32, the half sizes, the clamped radius, A
// - R and B - R, the floored sigma, 1 / (sigma sqrt 2), the cap window K sigma, and N and K.
type ShadPlan struct {
	M                                                [6]int64
	Centre                                           [2]int64
	A, B, Radius, Core, Straight, Sigma, InvS, Window float32
	N, K                                             uint32
}

func (desc ShadowDesc) c() C.jh_shadow_desc {
	d := C.jh_shadow_desc{x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height),
		flags: C.uint32_t(desc.Flags), radius: C.float(desc.Radius), sigma: C.float(desc.Sigma)}
	for i, m := range desc.Matrix {
		d.matrix[i] = C.double(m)
	}
	for i := 0; i < 4; i++ {
		d.box[i], d.color[i] = C.float(desc.Box[i]), C.float(desc.Color[i])
	}
	return d
}

// ShadowPlan is jh_shadow_plan: the plan of desc -- with the bounds the only place binary64 appears in the shadow rule.  Host only.
func ShadowPlan(desc ShadowDesc) (ShadPlan, error) {
	d := desc.c()
	var p C.jh_shad_plan
	if C.jh_shadow_plan(&d, &p) != 0 {
		return ShadPlan{}, fmt.Errorf("hip_engine: ShadowPlan: a descriptor the rule refuses")
	}
	out := ShadPlan{A: float32(p.a), B: float32(p.b), Radius: float32(p.radius), Core: float32(p.core), Straight: float32(p.straight),
		Sigma: float32(p.sigma), InvS: float32(p.inv_s), Window: float32(p.window), N: uint32(p.n), K: uint32(p.k)}
	for i := 0; i < 6; i++ {
		out.M[i] = int64(p.m[i])
	}
	out.Centre[0], out.Centre[1] = int64(p.centre[0]), int64(p.centre[1])
	return out, nil
}

// ShadowBounds is jh_shadow_bounds: the rectangle (x, y, width, height) of a dstW x dstH destination outside which the coverage is
// below 2^-12 -- what the rectangle of a ShadowDesc is restricted to; all zero when nothing is left.  Host only.
func ShadowBounds(desc ShadowDesc, dstW, dstH uint32) ([4]uint32, error) {
	d := desc.c()
	var r [4]C.uint32_t
	if C.jh_shadow_bounds(&d, C.uint32_t(dstW), C.uint32_t(dstH), &r[0]) != 0 {
		return [4]uint32{}, fmt.Errorf("hip_engine: ShadowBounds: a descriptor the rule refuses or an image extent above 2^23")
	}
	return [4]uint32{uint32(r[0]), uint32(r[1]), uint32(r[2]), uint32(r[3])}, nil
}

// Shadow is jh_shadow: the Gaussian blur of a rounded rectangle times a colour, GENERATED into the RGBA16F image dst or, with
// ShadowOver, laid over what it holds, by the rule of DESIGN.md 5.18 (defined on values: every implementation gives the same bits).
// Stream-ordered behind the frame, waits for nothing, one kernel launch whose cost does not depend on sigma, no scratch and no
// tables: always capturable.
func (e *Engine) Shadow(dst renderer.ImageProxy, desc ShadowDesc) {
	d := desc.c()
	e.check(C.jh_shadow(e.ctx, C.uint64_t(dst.ID), &d), "shadow")
}

// PerspectiveStraight is JH_PERSPECTIVE_STRAIGHT: the source's four channels are filtered as stored, not colour times alpha.
const PerspectiveStraight uint32 = 1

// PerspectiveDesc is jh_perspective_desc (include/jello_hip.h "Perspective"): WarpDesc's fields with WarpDesc's meaning, the matrix
// with nine entries, column-major: (a, b, p, c, d, q, e, f, s), x' w = a x + c y + e, y' w = b x + d y + f, w = p x + q y + s, from
// the source rectangle to the destination image.
type PerspectiveDesc struct {
	Matrix                          [9]float64
	Filter                          WarpFilter
	Edge                            WarpEdge
	Flags                           uint32
	SrcX, SrcY, SrcWidth, SrcHeight uint32
	DstX, DstY, DstWidth, DstHeight uint32
}

// PerspectivePlan is jh_perspective_plan: the nine doubles G of the perspective rule (DESIGN.md 5.19) -- the adjugate of the matrix
// scaled by a power of two so that every |G| <= 1, negated when the determinant is negative.  Host only.
func PerspectivePlan(matrix [9]float64) ([9]float64, error) {
	var m, g [9]C.double
	for i, v := range matrix {
		m[i] = C.double(v)
	}
	if C.jh_perspective_plan(&m[0], &g[0]) != 0 {
		return [9]float64{}, fmt.Errorf("hip_engine: PerspectivePlan: an illegal matrix")
	}
	var out [9]float64
	for i, v := range g {
		out[i] = float64(v)
	}
	return out, nil
}

// PerspectiveBounds is jh_perspective_bounds: the rectangle (x, y, width, height) of a dstW x dstH destination outside which
// Perspective of a srcW x srcH source rectangle under WarpEdgeZero is transparent black -- the whole destination when the rectangle
// reaches w <= 0; all zero when nothing is left.  Host only.
func PerspectiveBounds(matrix [9]float64, srcW, srcH uint32, filter WarpFilter, dstW, dstH uint32) ([4]uint32, error) {
	var m [9]C.double
	for i, v := range matrix {
		m[i] = C.double(v)
	}
	var r [4]C.uint32_t
	if C.jh_perspective_bounds(&m[0], C.uint32_t(srcW), C.uint32_t(srcH), C.int(filter), C.uint32_t(dstW), C.uint32_t(dstH), &r[0]) != 0 {
		return [4]uint32{}, fmt.Errorf("hip_engine: PerspectiveBounds: an illegal matrix, an unknown filter or a side above 32768")
	}
	return [4]uint32{uint32(r[0]), uint32(r[1]), uint32(r[2]), uint32(r[3])}, nil
}

// Perspective is jh_perspective: a rectangle of the RGBA16F image src under a projective map into a rectangle of the RGBA16F image dst
// (another image) by the rule of DESIGN.md 5.19 (defined on values: every implementation gives the same bits).  A CSS perspective()
// / rotateX / rotateY / matrix3d card flip, a keystone correction, a layer on an arbitrary quad.  A destination texel whose source
// lies behind the viewer is transparent black.  No minification prefilter: toward the horizon the result aliases.  Stream-ordered
// behind the frame, waits for nothing, one kernel launch, no scratch and no tables: always capturable.
func (e *Engine) Perspective(src, dst renderer.ImageProxy, desc PerspectiveDesc) {
	d := C.jh_perspective_desc{filter: C.int(desc.Filter), edge: C.int(desc.Edge), flags: C.uint32_t(desc.Flags),
		src_x: C.uint32_t(desc.SrcX), src_y: C.uint32_t(desc.SrcY), src_width: C.uint32_t(desc.SrcWidth), src_height: C.uint32_t(desc.SrcHeight),
		dst_x: C.uint32_t(desc.DstX), dst_y: C.uint32_t(desc.DstY), dst_width: C.uint32_t(desc.DstWidth), dst_height: C.uint32_t(desc.DstHeight)}
	for i, m := range desc.Matrix {
		d.matrix[i] = C.double(m)
	}
	e.check(C.jh_perspective(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "perspective")
}

// DistanceWhich is jh_distance_which: the distance to the nearest seed, to the nearest non-seed, or signed (negative inside).
type DistanceWhich int32

const (
	DistanceOuter  DistanceWhich = 0
	DistanceInner  DistanceWhich = 1
	DistanceSigned DistanceWhich = 2
)

// DistanceEdge is jh_distance_edge: every position outside the image is a non-seed, or none exists.
type DistanceEdge int32

const (
	DistanceEdgeZero  DistanceEdge = 0
	DistanceEdgeClamp DistanceEdge = 1
)

// DistanceStraight is JH_DISTANCE_STRAIGHT: f16(color v) is stored as it is, not by the store rule.
const DistanceStraight uint32 = 1

// DistanceDesc is jh_distance_desc (include/jello_hip.h "Distance"): the channel (0..3) and threshold that make a texel a seed, which
// distance, the edge mode, R = MaxDistance (1..255), the ramp v = clamp(s Scale + Offset, 0, 1), the premultiplied colour, the flags and
// the rectangle of dst that is written (0 x 0: the whole image).
type DistanceDesc struct {
	Channel             int32
	Threshold           float32
	Which               DistanceWhich
	Edge                DistanceEdge
	MaxDistance         uint32
	Scale, Offset       float32
	Color               [4]float32
	Flags               uint32
	X, Y, Width, Height uint32
}

func (desc DistanceDesc) c() C.jh_distance_desc {
	d := C.jh_distance_desc{channel: C.int(desc.Channel), threshold: C.float(desc.Threshold), which: C.int(desc.Which), edge: C.int(desc.Edge),
		max_distance: C.uint32_t(desc.MaxDistance), scale: C.float(desc.Scale), offset: C.float(desc.Offset), flags: C.uint32_t(desc.Flags),
		x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height)}
	for i, v := range desc.Color {
		d.color[i] = C.float(v)
	}
	return d
}

// DistPlan is jh_dist_plan: the resolved rectangle, R, CAP = (R + 1)^2, the planes of the intermediate and the scratch they take.
type DistPlan struct {
	X, Y, Width, Height     uint32
	Radius, Cap             uint32
	Planes                  uint32
	PlaneColumns, PlaneRows uint32
	ScratchBytes            uint64
}

// DistancePlan is jh_distance_plan: what Distance does with desc on an imageW x imageH image -- in particular the scratch bytes, which
// say which eager call has to precede a capture (one that needs no less).  Host only.
func DistancePlan(desc DistanceDesc, imageW, imageH uint32) (DistPlan, error) {
	d := desc.c()
	var p C.jh_dist_plan
	if C.jh_distance_plan(&d, C.uint32_t(imageW), C.uint32_t(imageH), &p) != 0 {
		return DistPlan{}, fmt.Errorf("hip_engine: DistancePlan: a descriptor the rule refuses or a rectangle the image refuses")
	}
	return DistPlan{X: uint32(p.x), Y: uint32(p.y), Width: uint32(p.width), Height: uint32(p.height), Radius: uint32(p.radius), Cap: uint32(p.cap),
		Planes: uint32(p.planes), PlaneColumns: uint32(p.plane_columns), PlaneRows: uint32(p.plane_rows), ScratchBytes: uint64(p.scratch_bytes)}, nil
}

// Distance is jh_distance: the Euclidean distance to the shape in the RGBA16F image src -- the texels whose channel is >= the threshold
// -- capped at MaxDistance, through a linear ramp, times a colour, into the image dst of the same size (dst may be src) by the rule of
// DESIGN.md 5.20 (defined on integers and on values: every implementation gives the same bits).  Round outlines, strokes of fractional
// width, disc dilate and erode, glows, SDF textures.  Stream-ordered behind the frame, waits for nothing, two kernel launches; the
// intermediate planes live in a scratch array that only grows, so the call is capturable once a call needing no less has run eagerly.
func (e *Engine) Distance(src, dst renderer.ImageProxy, desc DistanceDesc) {
	d := desc.c()
	e.check(C.jh_distance(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), &d), "distance")
}

// LoadAlpha is jh_load_alpha: byte 3 of a loaded surface pixel is straight alpha, the alpha the colour has been multiplied by (what
// RenderToSurface writes), or ignored (BGRX: the texel is opaque).
type LoadAlpha int32

const (
	LoadAlphaStraight      LoadAlpha = C.JH_LOAD_ALPHA_STRAIGHT
	LoadAlphaPremultiplied LoadAlpha = C.JH_LOAD_ALPHA_PREMULTIPLIED
	LoadAlphaOpaque        LoadAlpha = C.JH_LOAD_ALPHA_OPAQUE
)

// ChromaFilter is jh_chroma_filter: the chroma sample that covers the texel, or the 9 / 3 / 3 / 1 blend of the four nearest.
type ChromaFilter int32

const (
	ChromaReplicate ChromaFilter = C.JH_CHROMA_REPLICATE
	ChromaBilinear  ChromaFilter = C.JH_CHROMA_BILINEAR
)

// LoadSurface is jh_load_surface: the 8-bit frame at src (device memory, rows pitch bytes apart, in format) INTO the rectangle
// (x, y, width, height) of the RGBA16F image dst -- 0 x 0: the whole image; the frame has the rectangle's size -- by the rule of
// DESIGN.md 5.21 (defined on values: every implementation gives the same bits).  A decoded picture or a screen capture becomes the
// source of Composite, Warp, Perspective.  Stream-ordered behind the frame, waits for nothing, one kernel launch, no scratch and no
// tables: always capturable.
func (e *Engine) LoadSurface(dst renderer.ImageProxy, src unsafe.Pointer, pitch uint64, format SurfaceFormat, alpha LoadAlpha, x, y, width, height uint32) {
	d := C.jh_load_surface_desc{format: C.int32_t(format), alpha: C.int32_t(alpha), src: src, pitch: C.uint64_t(pitch), x: C.uint32_t(x), y: C.uint32_t(y),
		width: C.uint32_t(width), height: C.uint32_t(height)}
	e.check(C.jh_load_surface(e.ctx, C.uint64_t(dst.ID), &d), "load_surface")
}

// LoadYUV is jh_load_yuv: the 8-bit Y'CbCr 4:2:0 frame in planes (device memory, laid out as RenderToYUV writes them; the third is
// unused for NV12) INTO the rectangle of the RGBA16F image dst, opaque, by the rule of DESIGN.md 5.21: a decoded video frame becomes
// the source of Composite, Warp, Perspective.  format.Transfer says whether the R'G'B' codes are sRGB-encoded (decoded to linear)
// or linear.  Stream-ordered behind the frame, waits for nothing, one kernel launch, no scratch and no tables: always capturable.
func (e *Engine) LoadYUV(dst renderer.ImageProxy, planes [3]unsafe.Pointer, pitches [3]uint64, format YUVFormat, chroma ChromaFilter, x, y, width, height uint32) {
	d := C.jh_load_yuv_desc{layout: C.int32_t(format.Layout), matrix: C.int32_t(format.Matrix), _range: C.int32_t(format.Range),
		transfer: C.int32_t(format.Transfer), chroma: C.int32_t(chroma), x: C.uint32_t(x), y: C.uint32_t(y), width: C.uint32_t(width), height: C.uint32_t(height)}
	for i := 0; i < 3; i++ {
		d.plane[i] = planes[i]
		d.pitch[i] = C.uint64_t(pitches[i])
	}
	e.check(C.jh_load_yuv(e.ctx, C.uint64_t(dst.ID), &d), "load_yuv")
}

// StatsPopulation is jh_stats_population: the extremes and the histogram are taken over every texel of the rectangle, or over the
// content texels only.
type StatsPopulation int32

const (
	StatsAll     StatsPopulation = C.JH_STATS_ALL
	StatsContent StatsPopulation = C.JH_STATS_CONTENT
)

// StatsTransfer is jh_stats_transfer: the histogram's code for R, G, B (alpha is always linear).
type StatsTransfer int32

const (
	StatsLinear StatsTransfer = C.JH_STATS_LINEAR
	StatsSRGB   StatsTransfer = C.JH_STATS_SRGB
)

// The parts of the record (jh_stats_desc.what): any non-empty subset.
const (
	StatsBounds    uint32 = C.JH_STATS_BOUNDS
	StatsExtremes  uint32 = C.JH_STATS_EXTREMES
	StatsHistogram uint32 = C.JH_STATS_HISTOGRAM
)

// StatsRecordBytes is sizeof(jh_stats_record): what Stats writes at its out pointer.
const StatsRecordBytes = C.sizeof_jh_stats_record

// StatsDesc is jh_stats_desc (include/jello_hip.h "Stats"): the parts asked for, the channel (0..3) and threshold that make a texel
// content, the population, the histogram's transfer, and the rectangle of the image that is read (0 x 0: the whole image).
type StatsDesc struct {
	What                uint32
	Channel             int32
	Threshold           float32
	Population          StatsPopulation
	Transfer            StatsTransfer
	X, Y, Width, Height uint32
}

func (desc StatsDesc) c() C.jh_stats_desc {
	return C.jh_stats_desc{what: C.uint32_t(desc.What), channel: C.int(desc.Channel), threshold: C.float(desc.Threshold), population: C.int(desc.Population),
		transfer: C.int(desc.Transfer), x: C.uint32_t(desc.X), y: C.uint32_t(desc.Y), width: C.uint32_t(desc.Width), height: C.uint32_t(desc.Height)}
}

// StatsPlanResult is jh_stats_plan_t: the resolved rectangle, the kernel launches, the bytes of the record and of the scratch.
type StatsPlanResult struct {
	X, Y, Width, Height uint32
	Launches            uint32
	RecordBytes         uint64
	ScratchBytes        uint64
}

// StatsPlan is jh_stats_plan: what Stats does with desc on an imageW x imageH image.  Host only.
func StatsPlan(desc StatsDesc, imageW, imageH uint32) (StatsPlanResult, error) {
	d := desc.c()
	var p C.jh_stats_plan_t
	if C.jh_stats_plan(&d, C.uint32_t(imageW), C.uint32_t(imageH), &p) != 0 {
		return StatsPlanResult{}, fmt.Errorf("hip_engine: StatsPlan: a descriptor the rule refuses or a rectangle the image refuses")
	}
	return StatsPlanResult{X: uint32(p.x), Y: uint32(p.y), Width: uint32(p.width), Height: uint32(p.height), Launches: uint32(p.launches),
		RecordBytes: uint64(p.record_bytes), ScratchBytes: uint64(p.scratch_bytes)}, nil
}

// StatsCodes is jh_stats_codes: the histogram code of every f16 bit pattern of bits under transfer, as a colour channel's.  Host only.
func StatsCodes(transfer StatsTransfer, bits []uint16) ([]uint8, error) {
	codes := make([]uint8, len(bits))
	if len(bits) == 0 {
		return codes, nil
	}
	if C.jh_stats_codes(C.int(transfer), C.uint64_t(len(bits)), (*C.uint16_t)(unsafe.Pointer(&bits[0])), (*C.uint8_t)(unsafe.Pointer(&codes[0]))) != 0 {
		return nil, fmt.Errorf("hip_engine: StatsCodes: unknown transfer")
	}
	return codes, nil
}

// Stats is jh_stats: the content box, the channel extremes and four 256-bin histograms of a rectangle of the RGBA16F image src, as a
// jh_stats_record at out -- StatsRecordBytes of caller-owned device memory on an 8-byte boundary -- by the rule of DESIGN.md 5.22
// (integer counts, mins and maxes over the set of texels: every implementation gives the same bytes).  The box is the rectangle the
// other image calls take for a layer; the histogram chooses ColorFilter's functions.  The image is only read.  Stream-ordered behind
// the frame, waits for nothing, two kernel launches; the partial records live in a scratch array of one size for every image, so
// the call is capturable once one call has run eagerly.
func (e *Engine) Stats(src renderer.ImageProxy, desc StatsDesc, out unsafe.Pointer) {
	d := desc.c()
	e.check(C.jh_stats(e.ctx, C.uint64_t(src.ID), &d, out), "stats")
}

// Lut3DMinSize and Lut3DMaxSize are JH_LUT3D_MIN_SIZE and JH_LUT3D_MAX_SIZE: the sizes N of a 3D lookup table.
const (
	Lut3DMinSize = 2
	Lut3DMaxSize = 65
)

// Lut3DIdentity is jh_lut3d_identity: the identity table of n as the texels of its image -- n wide, n*n high, four f16 bit patterns
// per texel, entry (r, g, b) at (x = r, y = g + n b), value f16(index / (n - 1)), alpha 1.0.  Host only.
func Lut3DIdentity(n uint32) ([]uint16, error) {
	if n < Lut3DMinSize || n > Lut3DMaxSize {
		return nil, fmt.Errorf("hip_engine: Lut3DIdentity: size outside 2..65")
	}
	texels := make([]uint16, 4*int(n)*int(n)*int(n))
	if C.jh_lut3d_identity(C.uint32_t(n), (*C.uint16_t)(unsafe.Pointer(&texels[0]))) != 0 {
		return nil, fmt.Errorf("hip_engine: Lut3DIdentity: size outside 2..65")
	}
	return texels, nil
}

// Lut3D is jh_lut3d: the 3D colour lookup table held by the RGBA16F image lut -- size wide and size*size high, Lut3DIdentity's layout,
// the order of a .cube file -- applied by tetrahedral interpolation to the rectangle of the RGBA16F image src (0 x 0: the whole image)
// and written to the same rectangle of dst, by the rule of DESIGN.md 5.23: the colour clamped to [0, 1], four entries read per texel,
// alpha copied.  src may be dst and lut may be src; lut is never dst.  The table is an image like any other: UploadImage writes it, and
// ColorFilter calls over an identity table bake their chain into it.  Stream-ordered behind the frame, waits for nothing, one kernel
// launch, no scratch and no tables: always capturable.
func (e *Engine) Lut3D(src, dst, lut renderer.ImageProxy, size, x, y, width, height uint32) {
	d := C.jh_lut3d_desc{size: C.uint32_t(size), flags: 0, x: C.uint32_t(x), y: C.uint32_t(y), width: C.uint32_t(width), height: C.uint32_t(height)}
	e.check(C.jh_lut3d(e.ctx, C.uint64_t(src.ID), C.uint64_t(dst.ID), C.uint64_t(lut.ID), &d), "lut3d")
}

// UnpackTiles is jh_unpack_tiles: writes the SOLID and RAW tiles of the pack (device memory, packBytes long; untrusted: what
// fails the checks is ignored) into the frame at dst and touches nothing else.  Stream-ordered.
func (e *Engine) UnpackTiles(pack unsafe.Pointer, packBytes uint64, dst unsafe.Pointer, dstPitch uint64, width, height, texelBytes uint32) {
	e.check(C.jh_unpack_tiles(e.ctx, pack, C.uint64_t(packBytes), dst, C.uint64_t(dstPitch), C.uint32_t(width), C.uint32_t(height),
		C.uint32_t(texelBytes)), "unpack_tiles")
}

// ReadPack downloads the pack at pack (capacity bytes of device memory): the 32-byte header, then exactly the total size the
// header states.  These two small copies are the only host waits of the transport.
func (e *Engine) ReadPack(pack unsafe.Pointer, capacity uint64) []byte {
	e.check(C.jh_buffer_import(e.ctx, C.uint64_t(packBufferID), pack, C.uint64_t(capacity)), "buffer_import")
	defer C.jh_free(e.ctx, C.uint64_t(packBufferID)) // caller-owned memory: forgetting it frees nothing
	var h [8]uint32
	e.check(C.jh_download(e.ctx, C.uint64_t(packBufferID), unsafe.Pointer(&h[0]), 0, 32), "download")
	align16 := func(v uint64) uint64 { return (v + 15) &^ 15 }
	tb := uint64(h[3])
	total := 32 + align16(8*uint64(h[4])) + align16(tb*uint64(h[5])) + 256*tb*uint64(h[6])
	if h[0] != 0x3150544A || (tb != 4 && tb != 8) || uint64(h[5])+uint64(h[6]) != uint64(h[4]) || total > capacity {
		panic("hip_engine: ReadPack: not a pack, or larger than the capacity given")
	}
	out := make([]byte, total)
	e.check(C.jh_download(e.ctx, C.uint64_t(packBufferID), unsafe.Pointer(unsafe.SliceData(out)), 0, C.uint64_t(total)), "download")
	return out
}

// TrimScratch gives the context's internal scratch arrays back (the count / offset arrays of the deterministic allocators,
// flatten's temporary: they grow on demand and are kept).  For the frame after one that was much larger -- or after a first
// frame that ran with far more generous BumpSizes than the scenes need.  Waits for the stream.
func (e *Engine) TrimScratch() {
	e.check(C.jh_scratch_trim(e.ctx), "scratch_trim")
}

// SetBand: ONE target over several GPUs -- this engine then writes the PTCL and rasterises only the
// 256-pixel bin rows [row0, row1) of the target, with every allocation offset identical to the
// unsharded run (record the same Recording on every GPU; nothing else changes).
func (e *Engine) SetBand(row0, row1 uint32) {
	e.check(C.jh_set_band(e.ctx, C.uint32_t(row0), C.uint32_t(row1)), "set_band")
}

// SelfTest runs the library's toolchain checks on the device: the allocation patterns the kernels rely on (jh_selftest_atomics,
// forms 0 plain per-lane atomic / 1 hand-aggregated / 2 wave-private LDS) against a serial execution.  A deployment that rebuilds
// libjello_hip.so with another ROCm can call it once after New; it returns an error naming the form that disagrees.
func (e *Engine) SelfTest() error {
	for form := 0; form < 3; form++ {
		if rc := C.jh_selftest_atomics(e.ctx, C.int(form), C.uint32_t(1+form), 1024); rc != 0 {
			return fmt.Errorf("hip_engine: jh_selftest_atomics form %d: %d", form, int(rc))
		}
	}
	return nil
}
