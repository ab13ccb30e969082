// hip_engine.h -- replays a renderer Recording on an MI355X through the C ABI of
// include/jello_hip.h.  Drop-in for engine/wgpu_engine: Engine::run_recording mirrors
// RunRecording (wgpu.go:322-643) command by command, Engine::render_to_texture mirrors
// RenderToTexture (lib.go:244-264).  A Go `engine/hip_engine` package does the same walk through
// cgo; this C++ twin exists because the build image has no Go toolchain.
#pragma once
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "jello_hip.h"
#include "renderer.h"

namespace jello {

struct EngineError : std::runtime_error {
    int code;
    EngineError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

struct ExternalImage { ImageProxy proxy; void* device_ptr; };   // wgpu.go:90-93
struct ExternalBuffer { BufferProxy proxy; void* device_ptr; }; // wgpu.go:85-88

enum RunFlags : unsigned {
    kRunUploads = 1,     // Upload / UploadUniform / UploadImage
    kRunDispatches = 2,  // Dispatch / DispatchIndirect / Clear / Download
    kRunFrees = 4,       // FreeBuffer / FreeImage (deferred to the end of the recording, wgpu.go:601-616)
    kRunSkipFine = 8,    // with kRunDispatches: every dispatch but the fine stage's (the last one of a RenderFull recording)
    kRunOnlyFine = 16,   // with kRunDispatches: the fine stage's dispatch alone -- the two let a caller put fine on a stream of its own
    kRunAll = 7
};

class Engine {
   public:
    explicit Engine(int device);
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    jh_ctx* ctx() { return ctx_; }
    FullShaders& shaders() { return shaders_; }

    // RunRecording.  Buffers that the recording never frees stay resident (wgpu.go:631-640).
    void run_recording(const Recording& rec, const std::vector<ExternalImage>& images = {}, const std::vector<ExternalBuffer>& buffers = {},
                       unsigned flags = kRunAll);

    // RenderToTexture: record + run.  If `out_device` is non-null it must point to width*height*8
    // bytes of device memory (RGBA16F) and receives the image; otherwise the engine owns the target
    // and `download_target` reads it back.  robust=true re-runs with grown bump buffers while
    // bump.failed is set (the regrow loop Vello has and Jello lacks).
    struct Frame {
        Recording recording;
        RenderConfig config;
        ImageProxy target;
        std::map<std::string, BufferProxy> buffers;
        JlBump bump{};     // what the frame's Download(bumpBuf) returned: only a robust recording has one (all zero otherwise)
        int attempts = 1;
    };
    Frame render_to_texture(const Encoding& enc, RenderParams params, void* out_device = nullptr, bool robust = false, bool retain = false);
    void download_target(const Frame& f, void* dst, size_t bytes);
    void release(const Frame& f);  // frees whatever a retain=true frame kept

    // RenderToSurface (lib.go:266-333): render_to_texture into an engine-owned RGBA16F target -- kept while width and height
    // stay the same (eng.target, lib.go:279-284) -- then jh_blit into `surface`: device memory of height rows of 4 * width
    // bytes, `pitch` bytes apart, in the jh_surface_format `format`.  The frame's target image stays readable under
    // Frame::target.id until the next render_to_surface / render_to_yuv.
    Frame render_to_surface(const Encoding& enc, RenderParams params, void* surface, uint64_t pitch, int format, bool robust = true);
    // RenderToSurface for a video encoder: render_to_texture into the same engine-owned target, then jh_blit_yuv into the
    // planes of `desc` (NV12 / I420, include/jello_hip.h "YUV blit").  The frame's target image stays readable under
    // Frame::target.id until the next render_to_surface / render_to_yuv.
    Frame render_to_yuv(const Encoding& enc, RenderParams params, const jh_yuv_desc& desc, bool robust = true);

    // Downloads the tile pack (jh_pack_tiles; the format is in jello_hip.h) at device_ptr (capacity bytes of device memory): its
    // 32-byte header first, then exactly the total size the header states -- the only two host waits of the feature.  Returns
    // that size; throws when it exceeds capacity or out_capacity (a header that is not a pack's included).
    uint64_t read_pack(const void* device_ptr, uint64_t capacity, void* out, uint64_t out_capacity);

    Resolver& resolver() { return resolver_; }
    Renderer& renderer() { return renderer_; }

   private:
    void check(int rc, const char* what);
    jh_ctx* ctx_ = nullptr;
    // One group of the profile tree (pgroup.Nest(label); defer pgroup.End()): open for as long as the object lives.  A no-op
    // unless profiling is on.
    struct ProfileGroup {
        ProfileGroup(Engine& e, const char* label) : ctx(e.ctx_) { e.check(jh_profile_group_begin(ctx, label), "profile_group_begin"); }
        ~ProfileGroup() { (void)jh_profile_group_end(ctx); }
        ProfileGroup(const ProfileGroup&) = delete;
        jh_ctx* ctx;
    };
    Renderer renderer_;
    Resolver resolver_;
    FullShaders shaders_;
    std::map<ResourceID, std::vector<uint8_t>> downloads_;
    struct SurfaceTarget { ResourceID buffer = 0, image = 0; uint32_t width = 0, height = 0; };
    // render_to_texture into the engine's own target (created or resized first; the previous frame's image forgotten)
    Frame render_to_own_target(const Encoding& enc, const RenderParams& params, bool robust);
    SurfaceTarget surface_target_;  // render_to_surface's RGBA16F target (a context buffer) and the last frame's image over it

   public:
    const std::vector<uint8_t>* get_download(ResourceID id) const {
        auto it = downloads_.find(id);
        return it == downloads_.end() ? nullptr : &it->second;
    }
};

}  // namespace jello
