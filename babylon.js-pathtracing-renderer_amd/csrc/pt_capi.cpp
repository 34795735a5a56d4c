// pt_capi.cpp — one device's part of a libpt context (pt_dev.h): contexts, effects, textures,
// render targets and draws on one gfx950 device, mirroring the Babylon effect API the reference's
// setup scripts call. The exported C ABI (include/pt.h, pt_group.cpp) drives one such part per device
// of a context and fans every call out over them.
//
// What happens on dev_render(effect, target), per recognised program:
//   path tracing    -> (Cornell, quadrics, sky, sky + mesh, HDRI, glTF) uniforms resolved by name and
//                      SetupScene() evaluated once on the host with the same IEEE ops as the GLSL
//                      (trace_args), then the context's schedule over the 16-row bands it owns
//                      (dev_set_row_partition). The megakernel, the default (draw_mega): pt_trace, with
//                      late-bounce compaction the record sort and pt_cont, on one of the side streams,
//                      up to `depth` frames in flight, each gated by a mark on the main stream; then
//                      pt_blend on the main stream, and the longest-first order build deferred into the
//                      next screenOutput; with feature targets bound (dev_set_feature_targets) pt_trace also
//                      stages its G-buffer and pt_feature_fold follows the blend. Which buffer set, stream
//                      and mark, the grid and whether the draw compacts is pt_plan.h's arithmetic; this
//                      file reserves memory and issues the HIP calls. The wavefront and persistent schedules (draw_queued) run on the
//                      main stream alone;
//   SCREEN_COPY     -> pt_copy over the owned bands, deferred to fuse with the next screenOutput;
//   SCREEN_OUTPUT   -> pt_output into the canvas (RGBA8) or an RGBA32F target, with a deferred copy
//                      and order build riding along.
// The main stream is the context's own or the caller's (dev_set_stream); per-draw timing events are off
// until asked for (pt_last_render_ms, the timing window).
#include "../../include/pt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "pt_args.h"
#include "pt_knobs.h"
#include "pt_plan.h"
#include "pt_dev.h"

extern "C" {
hipError_t pt_launch_exhaustive(int op, unsigned long long* bad, hipStream_t s);
hipError_t pt_launch_trace(int prog, int count, const pt::TraceArgs* a, int grid_x, int grid_y, hipStream_t s);
hipError_t pt_launch_order_build(const pt::OrderArgs* a, hipStream_t s);
hipError_t pt_launch_copy(const pt::CopyArgs* a, int grid_x, int grid_y, hipStream_t s);
hipError_t pt_launch_blend(const pt::BlendArgs* a, int bands, hipStream_t s, int waves);
hipError_t pt_launch_feature_fold(const pt::FoldArgs* a, int bands, hipStream_t s, int waves);
hipError_t pt_launch_cont_sort(const pt::SortArgs* a, size_t cap, hipStream_t s);
hipError_t pt_launch_cont(int prog, const pt::TraceArgs* a, int waves, hipStream_t s);
hipError_t pt_launch_output(const pt::OutputArgs* a, hipStream_t s, int waves);
hipError_t pt_launch_math_probe(int op, const float* x, const float* y, float* out, int n, hipStream_t s);
hipError_t pt_launch_persist(int prog, int count, const pt::TraceArgs* a, const pt::WfBufs* w, int tiles_x,
                             unsigned n_wave_tiles, unsigned per_wave, unsigned refill, hipStream_t s);
hipError_t pt_launch_finish(const pt::TraceArgs* a, const pt::WfBufs* w, int tiles_x, int bands, hipStream_t s);
hipError_t pt_launch_pairs_pass(int pass, const float4* aabb, long long texels, const float4* tri, long long tri_texels,
                                unsigned nrec, unsigned char* inner, unsigned char* leafref, unsigned* counts,
                                float* code, float4* inner_rec, float4* leaf_rec, unsigned leaf_base, unsigned* bad,
                                hipStream_t s);
hipError_t pt_launch_wavefront(int prog, int count, const pt::TraceArgs* a, const pt::WfBufs* w, int tiles_x, int bands,
                               int persist_blocks, hipStream_t s);
hipError_t pt_launch_trail_pass(int pass, const float4* aabb, long long texels, unsigned nrec, const unsigned char* inner,
                                unsigned* parent, unsigned* refs, unsigned* flag, const float4* rec, uint32_t root,
                                float4* top, hipStream_t s);
}

#ifdef PT_SECPROF
#define PT_SECPROF_BUILD true
#else
#define PT_SECPROF_BUILD false
#endif

namespace {

enum TexKind { TEX_F32 = 0, TEX_U8 = 1, TEX_RT = 2 };
constexpr int kProgSlots = 9;

struct Uniform {
    int n = 0;
    bool is_int = false;
    bool set = false;
    float f[16] = {};
    int i = 0;
};

}  // namespace

struct DevTex {
    Dev* ctx = nullptr;
    int kind = TEX_F32;
    int w = 0, h = 0;
    void* d = nullptr;
    size_t bytes = 0;
    int sampling = PT_SAMPLING_NEAREST;
    int invert_y = 0;
    bool external = false;   // caller-owned device memory (dev_render_target_wrap)
    unsigned long long gen = 0;   // bumped by every host write of the texels
    // child-pair BVH records derived from this texture and the triangle texture drawn with it
    // (pt_pairs_* passes), valid while both keep the generations they were built from
    void* pairs_mem = nullptr;
    const float4* pairs_inner = nullptr;
    const float4* pairs_leaf = nullptr;
    uint32_t pairs_root = 0;
    float pairs_root_box[6] = {};
    uint32_t pairs_bytes = 0;   // inner records, then leaf records from pairs_leaf on, then the jump table
    uint32_t pairs_top = 0;     // byte offset of the restart-trail jump table; 0: the tree is not walkable by the trail
    const DevTex* pairs_tri = nullptr;
    unsigned long long pairs_gen = ~0ull, pairs_tri_gen = ~0ull;
    bool pairs_ok = false;
};

struct DevFx {
    Dev* ctx = nullptr;
    int prog = PT_PROG_UNKNOWN;
    std::unordered_map<std::string, Uniform> uniforms;
    std::unordered_map<std::string, DevTex*> samplers;
    DevTex* feat[2] = {};   // feature targets (dev_set_feature_targets): normal + id, albedo + weight
};

struct Dev {
    int device = 0;
    hipStream_t stream = nullptr;      // the stream all work is enqueued on
    hipStream_t own_stream = nullptr;  // the context's own stream (dev_set_stream(NULL) restores it)
    std::string err;
    uchar4* canvas = nullptr;
    int cw = 0, ch = 0;
    unsigned* d_err = nullptr;
    unsigned long long* d_counters = nullptr;
    bool counting = false;
    int num_parts = 1, part = 0;
    bool output_partition = false;
    // screenCopy deferred to ride along with the next screenOutput of the same source (flushed as
    // its own kernel before anything else could observe the target: flush_copy)
    struct { bool on; DevTex* src; DevTex* dst; int num_parts, part; } pending_copy = {};
    bool canvas_external = false;     // dev_canvas_wrap: caller-owned canvas memory
    pt::Knobs k;                      // the tunables, read from the environment once (pt_knobs.h)
    int backend = PT_BACKEND_MEGAKERNEL;
    int bvh_layout = PT_BVH_PAIRS;    // (k.bvh_layout at first; pt_set_bvh_layout)
    int bvh_used = -1;
    int cu_count = 256;
    pt::WfBufs wf = {};
    void* wf_mem = nullptr;
    size_t wf_pixels = 0, wf_slots = 0, wf_spill = 0;
    float2* mk_spill = nullptr;   // megakernel BVH stack spill slabs (one per side stream of the overlap depth)
    size_t mk_spill_lanes = 0;
    // Frame overlap (megakernel draws; k.overlap). pt_trace never reads the history:
    // it writes radiance + the pre-history flag to its buffer set's rad, and pt_blend folds in the
    // history on the main stream. So draw k's path tracing runs on side stream ts[k % depth] and waits
    // only for the main stream's state when an earlier draw began (with depth 2: draw k - 1's mark, i.e.
    // draw k - 2's blend, its order build, the output that read rad / the order), never for draw k - 1's
    // kernel: consecutive frames' path tracing overlap, and the next frame's waves fill the launch tail
    // of this one. Per buffer set: the radiance buffer, the compaction records and the longest-first
    // cost / order / split (each set is its own longest-first pipeline, draw k ordered by the costs of
    // the set's previous draw); per side stream: the spill slab.
    // Depth (k.depth, 2-6): side streams; draw k waits for the mark draw k - depth - lag + 1
    // recorded (depth 2, lag 0: the previous draw's), so up to `depth` frames' path tracing are in flight.
    static constexpr int kDepthMax = pt::kDepthMax;
    // Lag (k.lag): buffer sets beyond the streams. Draw k's buffer set is k % (depth + lag)
    // (radiance, compaction records, longest-first cost / order: what the main stream's blend, output
    // and order build read) and its stream / spill slab k % depth (what only its own stream touches),
    // and it waits for the mark of draw k - depth - lag + 1: with lag > 0 a side stream runs its next
    // draw as soon as its previous one ends, not after that draw's blend and output on the main stream.
    // By default (lag -1) the lag is kLagSmall for draws that trace fewer than k.lag_pixels pixels and
    // 0 above.
    static constexpr int kLagMax = pt::kLagMax, kSetsMax = kDepthMax + kLagMax;
    hipStream_t ts[kDepthMax] = {};
    hipEvent_t ev_mark[kSetsMax] = {}, ev_traced[kDepthMax] = {};
    pt::Overlap ov;               // which draw this is, its buffer set, stream and mark (pt_plan.h)
    float4* rad_mem = nullptr;    // rad[sets()]: radiance + flag per pixel
    size_t rad_pixels = 0;
    // feature buffers: feat[sets()][2] planes of a float4 per pixel beside rad (the G-buffer pt_trace stages for
    // pt_feature_fold), allocated once a draw has feature targets bound
    float4* feat_mem = nullptr;
    size_t feat_pixels = 0;
    // late-bounce compaction of the megakernel's mesh draws (pt_trace<P,false,true> -> pt_cont; k.cont_mode):
    // per buffer set 64-B path records, their pixels and a counter
    void* cont_mem = nullptr;
    size_t cont_cap = 0;          // records per buffer set ...
    int cont_sets = 0;            // ... and buffer sets allocated
    uint64_t cont_stored = 0;     // records stored by draws of earlier allocations (pt_cont_stats; cont_reserve)
    pt::ContTrial trial;          // auto mode: the draws of one target time it on and off (pt_plan.h)
    hipEvent_t tune_ev[2 * pt::kContBlocks] = {};   // ... by these events on the main stream
    int cont_last = 0;   // what the last megakernel draw did (pt::ContTrial::Draw::code)
    unsigned cont_draws = 0;   // megakernel draws that launched pt_cont, since the context was created
    pt::WfBufs gb = {};           // persistent backend: per-pixel G-buffer + radiance
    void* gb_mem = nullptr;
    size_t gb_pixels = 0;
    // the order build of the last megakernel draw (longest-first dispatch: cost[] / order[] of a path-tracing
    // draw, reused when the set's next draw has the same grid, target and program), deferred to run as an
    // extra block of the next screenOutput pass (pt_output) instead of a kernel of its own; any other draw,
    // stream switch or query launches it alone first (flush_order). k.fuse_order 0: always alone, after the draw.
    bool order_pending = false;
    pt::OrderArgs pending_order = {};
    unsigned* lpt_mem = nullptr;            // cost[kSetsMax][4 * cap] | order[kSetsMax][cap] | split[kSetsMax]
    size_t lpt_cap = 0;
    struct LptKey { bool valid; size_t n; const void* target; int prog, part, parts; };
    LptKey lpt_key[kSetsMax] = {};          // what cost[p] / order[p] were last written for
    unsigned* lpt_cost(int p) const { return lpt_mem + 4 * lpt_cap * p; }
    unsigned* lpt_order(int p) const { return lpt_mem + 4 * lpt_cap * kSetsMax + lpt_cap * p; }
    unsigned* lpt_split(int p) const { return lpt_mem + 5 * lpt_cap * kSetsMax + p; }
    int sets() const { return k.depth + (k.lag >= 0 ? k.lag : pt::kLagSmall); }   // buffer sets allocated (rad, compaction records)
    // per-draw events for pt_last_render_ms: off until its first call (or k.draw_events)
    bool draw_events = false;
    hipEvent_t ev0[kProgSlots] = {}, ev1[kProgSlots] = {};
    bool ev_used[kProgSlots] = {};
    // timing window: per draw event pairs, reused across windows; every timing_every-th draw of a
    // program kind is bracketed (PT_TIMING_EVERY, default 1 = every draw)
    bool window = false, window_rec = false;
    int timing_every = 1;
    int window_seen[kProgSlots] = {};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::vector<std::pair<int, int>> window_draws;   // (program, pool index)
    int pending = -1;
    std::set<DevTex*> textures;
    std::set<DevFx*> effects;
};

namespace {

int fail(Dev* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

int hipfail(Dev* c, hipError_t e, const char* what)
{
    return fail(c, PT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(c, call)                                   \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hipfail(c, e_, #call); \
    } while (0)

bool contains(const char* s, const char* pat) { return s && std::strstr(s, pat) != nullptr; }

// Recognise the program from the GLSL registered in Effect.ShadersStore (the reference passes
// `BABYLON.Effect.ShadersStore["...FragmentShader"]` as `fragmentShader`).
int classify(const char* src)
{
    if (contains(src, "uniform sampler2D pathTracedImageBuffer")) return PT_PROG_SCREEN_COPY;
    if (contains(src, "uniform sampler2D accumulationBuffer")) return PT_PROG_SCREEN_OUTPUT;
    if (!contains(src, "pathtracing_default_main")) return PT_PROG_UNKNOWN;
    if (contains(src, "uniform sampler2D tHDRTexture")) return PT_PROG_HDRI;
    if (contains(src, "uniform mat4 uTorusInvMatrix")) return PT_PROG_QUADRIC;
    if (contains(src, "pathtracing_physical_sky_functions"))   // the sky scene, or its composite with the
        return contains(src, "uniform sampler2D tAABBTexture") ? PT_PROG_SKY_MESH : PT_PROG_SKY;   // glTF model block
    if (contains(src, "uniform sampler2D tAABBTexture")) return PT_PROG_GLTF;
    if (contains(src, "uniform int uRightSphereMatType")) return PT_PROG_CORNELL;
    return PT_PROG_UNKNOWN;
}

float uf(const DevFx* fx, const char* name, int k = 0)
{
    auto it = fx->uniforms.find(name);
    if (it == fx->uniforms.end() || !it->second.set) return 0.0f;   // GLSL uniforms default to 0
    const Uniform& u = it->second;
    if (u.is_int) return (float)u.i;
    return k < u.n ? u.f[k] : 0.0f;
}
int ui(const DevFx* fx, const char* name)
{
    auto it = fx->uniforms.find(name);
    if (it == fx->uniforms.end() || !it->second.set) return 0;
    const Uniform& u = it->second;
    return u.is_int ? u.i : (int)u.f[0];
}
void um4(const DevFx* fx, const char* name, ptg::m4& m)
{
    for (int k = 0; k < 16; k++) m.m[k] = uf(fx, name, k);
}
DevTex* sampler(const DevFx* fx, const char* name)
{
    auto it = fx->samplers.find(name);
    return it == fx->samplers.end() ? nullptr : it->second;
}

pt::Tex8 tex8(const DevTex* t)
{
    pt::Tex8 r{ nullptr, 0, 0 };
    if (t && t->kind == TEX_U8) { r.p = (const uchar4*)t->d; r.w = t->w; r.h = t->h; }
    return r;
}

ptg::f3 v3(float x, float y, float z) { return ptg::f3{ x, y, z }; }
pt::QuadArg quad(ptg::f3 n, ptg::f3 a, ptg::f3 b, ptg::f3 c, ptg::f3 d, ptg::f3 col, int type)
{
    pt::QuadArg q;
    q.normal = n; q.v0 = a; q.v1 = b; q.v2 = c; q.v3 = d; q.color = col; q.type = type;
    return q;
}
float hdist(ptg::f3 a, ptg::f3 b)
{
    float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return std::sqrt(x * x + y * y + z * z);
}

// The uniform-only terms of Get_Sky_Color (js/PathTracingCommon.js:373-475) with the pinned
// sequences of pt_glsl.h, once per draw instead of once per sky sample
void sky_setup(const DevFx* fx, pt::SkyArgs& k)
{
    using namespace ptg;
    k.sun = v3(uf(fx, "uSunDirection", 0), uf(fx, "uSunDirection", 1), uf(fx, "uSunDirection", 2));
    const float cosSunUpAngle = dot(mk(0.0f, 1.0f, 0.0f), k.sun);
    const float z = gclamp(cosSunUpAngle, -1.0f, 1.0f);   // SunIntensity
    k.sunE = 200.0f * gmax(0.0f, 1.0f - gpow(2.71828182845904524f, -((1.6110731556870734f - gacos(z)) / 1.5f)));
    k.sunE19000 = k.sunE * 19000.0f;
    k.rayleigh = mk(5.804542996261093E-6f, 1.3562911419845635E-5f, 3.0265902468824876E-5f) * 2.0f;
    const float c = (0.2f * 0.5f) * 10E-18f;               // totalMie
    k.mie = (mk(1.8399918514433978E14f, 2.7798023919660528E14f, 4.0790479543861094E14f) * (0.434f * c)) * 0.03f;
    k.rm = k.rayleigh + k.mie;
    k.fade = gclamp(gpow(1.0f - cosSunUpAngle, 5.0f), 0.0f, 1.0f);
    const float sunfade = 1.0f - gclamp(1.0f - gexp((k.sun.y / 450000.0f)), 0.0f, 1.0f);
    k.retExp = 1.0f / (1.2f + (1.2f * sunfade));
}

// SetupScene() of js/BabylonPathTracing_FragmentShader.js:348-378 and
// js/GLTFModelPathTracing_FragmentShader.js:613-643, evaluated once per draw.
void setup_scene(const DevFx* fx, pt::TraceArgs& a)
{
    const float W = 50.0f;
    const float L = uf(fx, "uQuadLightRadius") * 0.2f;
    const ptg::f3 E = v3(1.0f * 10.0f, 1.0f * 10.0f, 1.0f * 10.0f);
    const ptg::f3 white = v3(1.0f, 1.0f, 1.0f);
    um4(fx, "uLeftSphereInvMatrix", a.sph[0].inv);
    um4(fx, "uRightSphereInvMatrix", a.sph[1].inv);
    a.sph[0].color = v3(1.0f, 1.0f, 0.0f);
    a.sph[0].type = pt::CLEARCOAT_DIFFUSE;
    a.sph[1].color = v3(1.0f, 1.0f, 1.0f);
    const bool gltf = fx->prog == PT_PROG_GLTF || fx->prog == PT_PROG_HDRI;
    a.sph[1].type = gltf ? pt::METAL : ui(fx, "uRightSphereMatType");
    pt::QuadArg q[6];
    q[0] = quad(v3(0, 0, 1), v3(-W, W, W), v3(W, W, W), v3(W, -W, W), v3(-W, -W, W), white, pt::DIFFUSE);
    q[1] = quad(v3(1, 0, 0), v3(-W, -W, W), v3(-W, -W, -W), v3(-W, W, -W), v3(-W, W, W), v3(0.7f, 0.05f, 0.05f), pt::DIFFUSE);
    q[2] = quad(v3(-1, 0, 0), v3(W, -W, -W), v3(W, -W, W), v3(W, W, W), v3(W, W, -W), v3(0.05f, 0.05f, 0.7f), pt::DIFFUSE);
    q[3] = quad(v3(0, -1, 0), v3(-W, W, -W), v3(W, W, -W), v3(W, W, W), v3(-W, W, W), white, pt::DIFFUSE);
    q[4] = quad(v3(0, 1, 0), v3(-W, -W, W), v3(W, -W, W), v3(W, -W, -W), v3(-W, -W, -W), white, pt::DIFFUSE);
    const float sel = uf(fx, "uQuadLightPlaneSelectionNumber");
    const float wm = W - 1.0f, wp = -W + 1.0f;
    std::memset(&q[5], 0, sizeof(q[5]));   // unselected: the GLSL global keeps its zero default
    if (sel == 1.0f) q[5] = quad(v3(-1, 0, 0), v3(wm, -L, L), v3(wm, L, L), v3(wm, L, -L), v3(wm, -L, -L), E, pt::LIGHT);
    else if (sel == 2.0f) q[5] = quad(v3(1, 0, 0), v3(wp, -L, -L), v3(wp, L, -L), v3(wp, L, L), v3(wp, -L, L), E, pt::LIGHT);
    else if (sel == 3.0f) q[5] = quad(v3(0, 0, 1), v3(-L, -L, wp), v3(L, -L, wp), v3(L, L, wp), v3(-L, L, wp), E, pt::LIGHT);
    else if (sel == 4.0f) q[5] = quad(v3(0, 0, -1), v3(-L, -L, wm), v3(-L, L, wm), v3(L, L, wm), v3(L, -L, wm), E, pt::LIGHT);
    else if (sel == 5.0f) q[5] = quad(v3(0, 1, 0), v3(-L, wp, -L), v3(-L, wp, L), v3(L, wp, L), v3(L, wp, -L), E, pt::LIGHT);
    else if (sel == 6.0f) q[5] = quad(v3(0, -1, 0), v3(-L, wm, -L), v3(L, wm, -L), v3(L, wm, L), v3(-L, wm, L), E, pt::LIGHT);
    auto sub = [](ptg::f3 x, ptg::f3 y) { return v3(x.x - y.x, x.y - y.y, x.z - y.z); };
    for (int i = 0; i < 6; i++) {
        a.qtri[2 * i] = pt::TriArg{ q[i].v0, sub(q[i].v1, q[i].v0), sub(q[i].v2, q[i].v0) };
        a.qtri[2 * i + 1] = pt::TriArg{ q[i].v0, sub(q[i].v2, q[i].v0), sub(q[i].v3, q[i].v0) };
        a.qnormal[i] = q[i].normal;
        a.qcolor[i] = q[i].color;
        a.qtype[i] = q[i].type;
    }
    a.light = q[5];
    a.light_r2 = hdist(q[5].v0, q[5].v1) * hdist(q[5].v0, q[5].v3);
    a.nquads = 6;
    const bool sky = fx->prog == PT_PROG_SKY || fx->prog == PT_PROG_SKY_MESH;
    if (sky || fx->prog == PT_PROG_HDRI) {
        // js/PhysicalSkyModel_FragmentShader.js:383-399, js/HDRIEnvironmentPathTracing_FragmentShader.js:529-542:
        // N_QUADS 4 = back, left, right walls and the floor (the Cornell ceiling and quad light are gone)
        const pt::QuadArg floor = q[4];
        a.qtri[6] = pt::TriArg{ floor.v0, sub(floor.v1, floor.v0), sub(floor.v2, floor.v0) };
        a.qtri[7] = pt::TriArg{ floor.v0, sub(floor.v2, floor.v0), sub(floor.v3, floor.v0) };
        a.qnormal[3] = floor.normal;
        a.qcolor[3] = floor.color;
        a.qtype[3] = floor.type;
        a.nquads = 4;
    }
    if (sky) sky_setup(fx, a.sky);
    if (fx->prog == PT_PROG_QUADRIC) {   // js/TransformedQuadricGeometry_FragmentShader.js:9-24
        static const char* const kShapes[12] = {
            "uSphereInvMatrix", "uCylinderInvMatrix", "uConeInvMatrix", "uParaboloidInvMatrix",
            "uHyperboloidInvMatrix", "uCapsuleInvMatrix", "uFlattenedRingInvMatrix", "uBoxInvMatrix",
            "uPyramidFrustumInvMatrix", "uDiskInvMatrix", "uRectangleInvMatrix", "uTorusInvMatrix" };
        for (int k = 0; k < 12; k++) um4(fx, kShapes[k], a.shape_inv[k]);
        a.shape_k = uf(fx, "uShapeK");
        a.shape_mat = ui(fx, "uAllShapesMatType");
    }
    if (fx->prog == PT_PROG_HDRI) {
        a.sky.sun = v3(uf(fx, "uSunDirection", 0), uf(fx, "uSunDirection", 1), uf(fx, "uSunDirection", 2));
        a.hdr_exposure = uf(fx, "uHDRExposure");
        const float p = uf(fx, "uSunPower");
        a.sun_weight = p * p * 0.0000001f;
        const DevTex* h = sampler(fx, "tHDRTexture");
        if (h && h->kind != TEX_U8) { a.hdr.p = (const float4*)h->d; a.hdr.w = h->w; a.hdr.h = h->h; }
    }
}

int bands_owned(const Dev* c, int height) { return pt::bands_owned(height, c->num_parts, c->part); }

int begin_draw(Dev* c, int prog, hipStream_t s = nullptr)
{
    if (!s) s = c->stream;
    if (c->draw_events) {
        if (!c->ev0[prog]) {
            HIPCHK(c, hipEventCreate(&c->ev0[prog]));
            HIPCHK(c, hipEventCreate(&c->ev1[prog]));
        }
        HIPCHK(c, hipEventRecord(c->ev0[prog], s));
    }
    c->window_rec = c->window && c->window_seen[prog]++ % c->timing_every == 0;
    if (c->window_rec) {
        size_t k = c->window_draws.size();
        if (k == c->pool.size()) {
            hipEvent_t a, b;
            HIPCHK(c, hipEventCreate(&a));
            HIPCHK(c, hipEventCreate(&b));
            c->pool.emplace_back(a, b);
        }
        HIPCHK(c, hipEventRecord(c->pool[k].first, s));
        c->window_draws.emplace_back(prog, (int)k);
    }
    return PT_OK;
}
int end_draw(Dev* c, int prog, hipStream_t s = nullptr)
{
    if (!s) s = c->stream;
    if (c->draw_events) {
        HIPCHK(c, hipEventRecord(c->ev1[prog], s));
        c->ev_used[prog] = true;
    }
    if (c->window_rec)
        HIPCHK(c, hipEventRecord(c->pool[c->window_draws.back().second].second, s));
    return PT_OK;
}

// Grow a device allocation: wait for the streams whose work may still use the old one, free it, allocate
// `bytes` and record its new size (0 while there is none). WAIT_ALL: the side streams' path tracing uses it too.
// `fresh`: the megakernel's draws use it, so the next one waits for everything before it (new memory).
enum SlabWait { WAIT_MAIN, WAIT_ALL };
template <class T>
int slab_grow(Dev* c, T*& mem, size_t& size, size_t new_size, size_t bytes, SlabWait wait, bool fresh)
{
    if (mem) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int p = 0; wait == WAIT_ALL && p < Dev::kDepthMax; p++)
            if (c->ts[p]) HIPCHK(c, hipStreamSynchronize(c->ts[p]));
        HIPCHK(c, hipFree(mem));
        mem = nullptr;
    }
    size = 0;
    HIPCHK(c, hipMalloc(&mem, bytes));
    size = new_size;
    if (fresh) c->ov.need_fresh = true;
    return PT_OK;
}

// (re)allocate the wavefront buffers for `tiles` 16x16 tiles of a wq x hq quad-rounded frame and
// a persistent grid of `blocks` blocks: one slab, carved into the WfBufs arrays
int wf_reserve(Dev* c, int wq, int hq, int tiles, int blocks)
{
    const unsigned cap = (unsigned)((tiles + pt::kShards - 1) / pt::kShards) * pt::kBlock;
    const size_t slots = (size_t)cap * pt::kShards;
    const size_t pixels = (size_t)wq * hq;
    const size_t spill = (size_t)(pt::kStackLevels - pt::kStackLds) * blocks * pt::kBlock;
    if (c->wf_mem && slots <= c->wf_slots && pixels <= c->wf_pixels && spill <= c->wf_spill) {
        c->wf.shard_cap = cap; c->wf.wq = wq; c->wf.hq = hq;
        return PT_OK;
    }
    const size_t f4s = slots * sizeof(float4), f4p = pixels * sizeof(float4);
    const size_t bytes = 4096 + 10 * f4s + 3 * f4p + slots * sizeof(unsigned) + spill * sizeof(float2) + 16 * 256;
    if (int rc = slab_grow(c, c->wf_mem, c->wf_slots, slots, bytes, WAIT_MAIN, false)) return rc;
    char* m = (char*)c->wf_mem;
    auto take = [&](size_t n) { char* r = m; m += pt::align256(n); return r; };
    c->wf.cnt = (unsigned*)take(4096);
    c->wf.bcnt = c->wf.cnt + 8 * pt::kShards;
    for (int k = 0; k < 2; k++) {
        c->wf.qA[k] = (float4*)take(f4s); c->wf.qB[k] = (float4*)take(f4s);
        c->wf.qC[k] = (float4*)take(f4s); c->wf.qD[k] = (float4*)take(f4s);
    }
    c->wf.hit0 = (float4*)take(f4s); c->wf.hit1 = (float4*)take(f4s);
    c->wf.gb0 = (float4*)take(f4p); c->wf.gb1 = (float4*)take(f4p); c->wf.rad = (float4*)take(f4p);
    c->wf.bvhq = (unsigned*)take(slots * sizeof(unsigned));
    c->wf.spill = (float2*)take(spill * sizeof(float2));
    c->wf_pixels = pixels; c->wf_spill = spill;
    c->wf.shard_cap = cap; c->wf.wq = wq; c->wf.hq = hq;
    return PT_OK;
}

constexpr size_t kSpillPerLane = pt::kStackLevels - pt::kStackLdsMin + 4;   // float2 per lane of one slab

// the megakernel's spill slabs, one per side stream (overlapping draws must not share one): stack
// levels kStackLdsMin..27, then up to 8 floats per lane for the G-buffer fields kept out of LDS
// (pt_trace.h); slab p starts at spill_slab(c, p)
int spill_reserve(Dev* c, size_t lanes)
{
    if (lanes <= c->mk_spill_lanes) return PT_OK;
    return slab_grow(c, c->mk_spill, c->mk_spill_lanes, lanes, (size_t)c->k.depth * lanes * kSpillPerLane * sizeof(float2),
                     WAIT_MAIN, true);
}
float2* spill_slab(Dev* c, int p) { return c->mk_spill + (size_t)p * c->mk_spill_lanes * kSpillPerLane; }

// rad[sets()] (pt_trace -> pt_blend) for a frame of `pixels`
int rad_reserve(Dev* c, size_t pixels)
{
    if (pixels <= c->rad_pixels) return PT_OK;
    return slab_grow(c, c->rad_mem, c->rad_pixels, pixels, (size_t)c->sets() * pixels * sizeof(float4), WAIT_MAIN, true);
}

// feat[sets()][2] (pt_trace -> pt_feature_fold) for a frame of `pixels`: same sets, same growth rule as rad
int feat_reserve(Dev* c, size_t pixels)
{
    if (pixels <= c->feat_pixels) return PT_OK;
    return slab_grow(c, c->feat_mem, c->feat_pixels, pixels, (size_t)c->sets() * 2 * pixels * sizeof(float4), WAIT_MAIN, true);
}

// the pixels a draw of `target` traces: the owned bands, a bound on its records, and about, for the measured
// thresholds (pt_plan.h: the two are not interchangeable)
size_t owned_pixels(const Dev* c, const DevTex* target) { return pt::owned_pixels(target->w, target->h, c->num_parts, c->part); }
size_t share_pixels(const Dev* c, const DevTex* target) { return pt::share_pixels(target->w, target->h, c->num_parts); }

// pt_cont's records for draws that trace up to `paths` pixels (a record per traced pixel at most), in `sets`
// buffer sets, each laid out by pt::ContLayout; the counters start at zero here, afterwards each draw's pt_blend
// zeroes its own. (Sized by the partition's pixels and the sets its draws cycle through, not the whole target
// times every set: a 4K frame's records are 0.53 GB per set.)
pt::ContLayout cont_layout(const Dev* c) { return pt::ContLayout(c->cont_cap, c->k.cont_sort != 0); }
// the records the draws of the current allocation stored: the buffer sets' running totals, which each draw's
// pt_blend keeps in its counter block (the main stream must be idle)
int cont_totals(Dev* c, uint64_t* sum)
{
    *sum = 0;
    const pt::ContLayout L = cont_layout(c);
    for (int p = 0; c->cont_mem && p < c->cont_sets; p++) {
        uint64_t v = 0;
        HIPCHK(c, hipMemcpy(&v, (char*)c->cont_mem + (size_t)p * L.bytes + L.total(), sizeof(v), hipMemcpyDeviceToHost));
        *sum += v;
    }
    return PT_OK;
}
int cont_reserve(Dev* c, size_t paths, int sets)
{
    if (paths <= c->cont_cap && sets <= c->cont_sets) return PT_OK;
    paths = std::max(paths, c->cont_cap);
    sets = std::max(sets, c->cont_sets);
    if (c->cont_mem) {   // (the totals of the sets that go are carried over on the host)
        uint64_t stored = 0;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (int rc = cont_totals(c, &stored)) return rc;
        c->cont_stored += stored;
    }
    c->cont_sets = 0;
    const size_t bytes = (size_t)sets * pt::ContLayout(paths, c->k.cont_sort != 0).bytes;
    if (int rc = slab_grow(c, c->cont_mem, c->cont_cap, paths, bytes, WAIT_MAIN, true)) return rc;
    c->cont_sets = sets;
    // on the main stream (hipMemset would go to the null stream, which the non-blocking side streams do
    // not wait for: the next draw's atomics raced with it); the next draw's path tracing waits for a mark
    // recorded after it
    HIPCHK(c, hipMemsetAsync(c->cont_mem, 0, bytes, c->stream));
    return PT_OK;
}
// buffer set p's records as the draw's arguments; `sort`: with the arrays of the record sort (else NULL)
void cont_args(Dev* c, int p, bool sort, pt::TraceArgs& a)
{
    const pt::ContLayout L = cont_layout(c);
    char* m = (char*)c->cont_mem + (size_t)p * L.bytes;
    a.cont_rec = (float4*)(m + L.rec);
    a.cont_aux = (unsigned*)(m + L.aux);
    a.cont_count = (unsigned*)(m + L.count);
    a.cont_perm = sort ? (unsigned*)(m + L.perm) : nullptr;
    a.cont_rank = sort ? (unsigned*)(m + L.rank) : nullptr;
    a.cont_key = sort ? (unsigned short*)(m + L.key) : nullptr;
    a.cont_bins = sort ? (unsigned*)(m + L.bins) : nullptr;
    a.cont_bounce = (unsigned)c->k.cont_bounce;   // (>= 2: the G-buffer's normal / colour / id are final from bounce 2)
    a.cont_lanes = (unsigned)c->k.cont_lanes;
    a.cont_refill = (unsigned)c->k.cont_refill;
}

// Whether this draw compacts, and its frames in flight: pt::ContTrial decides; here the records, the auto trial's
// events on the main stream and the one wait at its end. `alone`: a moving-camera draw that runs alone (draw_mega).
int cont_decide(Dev* c, const DevTex* target, int prog, bool eligible, bool alone, pt::ContTrial::Draw* d)
{
    const size_t share = share_pixels(c, target);
    // the records first, so that no trial block pays for their allocation (for every set the draws of this
    // target cycle through: the depth, at most k.depth, plus the lag)
    if (eligible && c->k.cont_mode != 0)
        if (int rc = cont_reserve(c, owned_pixels(c, target), c->k.depth + pt::draw_lag(c->k, share))) return rc;
    *d = c->trial.draw({ target, prog, c->part, c->num_parts, target->w, target->h }, eligible, alone, share, c->k);
    if (d->event >= 0) {
        hipEvent_t& e = c->tune_ev[d->event];
        if (!e) HIPCHK(c, hipEventCreate(&e));
        HIPCHK(c, hipEventRecord(e, c->stream));
    }
    if (d->ends) {
        // the host waits for the trial once (the draws it has already queued ran without), so that every later
        // draw of this target takes the decision
        HIPCHK(c, hipEventSynchronize(c->tune_ev[2 * pt::kContBlocks - 1]));
        float ms[pt::kContBlocks] = {};
        for (int b = 0; b < pt::kContBlocks; b++) HIPCHK(c, hipEventElapsedTime(&ms[b], c->tune_ev[2 * b], c->tune_ev[2 * b + 1]));
        *d = c->trial.conclude(ms);
    }
    c->cont_last = d->code;
    return PT_OK;
}

// the side streams and events of frame overlap (created at the first overlapped draw)
int overlap_init(Dev* c)
{
    if (c->ts[0]) return PT_OK;
    for (int p = 0; p < c->sets(); p++) HIPCHK(c, hipEventCreateWithFlags(&c->ev_mark[p], hipEventDisableTiming));
    for (int p = 0; p < c->k.depth; p++) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->ts[p], hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_traced[p], hipEventDisableTiming));
    }
    return PT_OK;
}

int gb_reserve(Dev* c, int wq, int hq)
{
    const size_t pixels = (size_t)wq * hq;
    if (pixels > c->gb_pixels) {
        const size_t f4p = pt::align256(pixels * sizeof(float4));
        if (int rc = slab_grow(c, c->gb_mem, c->gb_pixels, pixels, 3 * f4p, WAIT_MAIN, false)) return rc;
        c->gb.gb0 = (float4*)c->gb_mem;
        c->gb.gb1 = (float4*)((char*)c->gb_mem + f4p);
        c->gb.rad = (float4*)((char*)c->gb_mem + 2 * f4p);
    }
    c->gb.wq = wq; c->gb.hq = hq;
    return PT_OK;
}

// The child-pair records of a BVH texture (with the triangle texture drawn alongside), rebuilt
// when either texture's texels changed since the last build. Only for data textures (their
// texels change only through this API) of at most 2^24 texels (node ids and ranks exact in
// float). Returns false when the reference walk must be used. One host round trip per build.
#ifdef PT_SECPROF
static unsigned long long* g_wave_log = nullptr;
static size_t g_wave_log_n = 0;
extern "C" __attribute__((visibility("default"))) size_t pt_debug_wave_log(unsigned long long* out, size_t n)
{
    hipDeviceSynchronize();
    n = n < g_wave_log_n ? n : g_wave_log_n;
    if (g_wave_log && n) hipMemcpy(out, g_wave_log, n * 8 * pt::kWaveLogSlots, hipMemcpyDeviceToHost);
    return n;
}
// the child-pair walk's load coherence since the last call (WalkStat, pt_device.h): 8 bounces x 5
// counters (wave iterations, record loads, uniform loads, loading lanes, lanes at the first lane's record)
static unsigned long long* g_walk_stat = nullptr;
extern "C" __attribute__((visibility("default"))) int pt_debug_walk_stats(unsigned long long out[40])
{
    hipDeviceSynchronize();
    if (!g_walk_stat) return -1;
    hipMemcpy(out, g_walk_stat, 40 * 8, hipMemcpyDeviceToHost);
    hipMemset(g_walk_stat, 0, 40 * 8);
    return 0;
}
#endif
bool ensure_pairs(Dev* c, DevTex* t, const DevTex* tri, int* rc)
{
    *rc = PT_OK;
    const long long texels = (long long)t->w * t->h;
    if (c->bvh_layout == PT_BVH_REFERENCE || t->kind != TEX_F32 || tri->kind != TEX_F32 || texels > (1ll << 24)) return false;
    if (t->pairs_gen == t->gen && t->pairs_tri == tri && t->pairs_tri_gen == tri->gen) return t->pairs_ok;
    if (t->pairs_mem) { hipStreamSynchronize(c->stream); hipFree(t->pairs_mem); t->pairs_mem = nullptr; }
    t->pairs_ok = false;
    t->pairs_top = 0;
    t->pairs_gen = t->gen; t->pairs_tri = tri; t->pairs_tri_gen = tri->gen;
    const unsigned nrec = (unsigned)((texels + 1) / 2);
    const unsigned nblk = (nrec + 1023) / 1024;
    constexpr auto al = pt::align256;
    unsigned char *inner = nullptr, *leafref = nullptr, *scratch = nullptr;
    unsigned* counts = nullptr;
    float* code = nullptr;
    unsigned *parent = nullptr, *refs = nullptr;   // restart-trail checks (pt_pairs_links / _depth)
    const size_t u4 = al(nrec * sizeof(unsigned));
    hipError_t e = hipMalloc(&scratch, 2 * al(nrec) + al(2 * nblk * sizeof(unsigned)) + al(nrec * sizeof(float)) + 2 * u4);
    std::vector<unsigned> h(2 * nblk);
    unsigned bad = 0, notrail = 0;
    if (e == hipSuccess) {
        inner = scratch; leafref = scratch + al(nrec);
        counts = (unsigned*)(scratch + 2 * al(nrec));
        code = (float*)((char*)counts + al(2 * nblk * sizeof(unsigned)));
        parent = (unsigned*)((char*)code + al(nrec * sizeof(float)));
        refs = (unsigned*)((char*)parent + u4);
        e = hipMemsetAsync(leafref, 0, nrec, c->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(refs, 0, nrec * sizeof(unsigned), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_err + 1, 0, 2 * sizeof(unsigned), c->stream);
    const float4* aabb = (const float4*)t->d;
    const float4* trid = (const float4*)tri->d;
    const long long ttex = (long long)tri->w * tri->h;
    unsigned leaf_base = 0;   // byte offset of the leaf records in the one record array
    auto pass = [&](int k, float4* ir, float4* lr) {
        return pt_launch_pairs_pass(k, aabb, texels, trid, ttex, nrec, inner, leafref, counts, code, ir, lr, leaf_base,
                                    c->d_err + 1, c->stream);
    };
    if (e == hipSuccess) e = pass(1, nullptr, nullptr);
    if (e == hipSuccess) e = pass(2, nullptr, nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), counts, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, c->d_err + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    size_t n_inner = 0, n_leaf = 0;
    if (e == hipSuccess && !bad) {
        for (unsigned b = 0; b < nblk; b++) {   // exclusive scan of the per-block counts
            unsigned ci = h[2 * b], cl = h[2 * b + 1];
            h[2 * b] = (unsigned)n_inner; h[2 * b + 1] = (unsigned)n_leaf;
            n_inner += ci; n_leaf += cl;
        }
        leaf_base = (unsigned)al(n_inner * 64);
        const size_t top_base = leaf_base + al(n_leaf * 48);
        const size_t rec_bytes = top_base + (size_t)pt::kTopEntries * 64;
        e = hipMalloc(&t->pairs_mem, rec_bytes + 256);
        if (e == hipSuccess) {
            t->pairs_inner = (const float4*)t->pairs_mem;
            t->pairs_leaf = (const float4*)((char*)t->pairs_mem + leaf_base);
            e = hipMemcpyAsync(counts, h.data(), h.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
        }
        if (e == hipSuccess) e = pass(3, nullptr, nullptr);
        if (e == hipSuccess) e = pass(4, (float4*)t->pairs_inner, (float4*)t->pairs_leaf);
        auto tpass = [&](int k, uint32_t root) {
            return pt_launch_trail_pass(k, aabb, texels, nrec, inner, parent, refs, c->d_err + 2, t->pairs_inner, root,
                                        (float4*)((char*)t->pairs_mem + top_base), c->stream);
        };
        if (e == hipSuccess) e = tpass(1, 0);
        if (e == hipSuccess) e = tpass(2, 0);
        float root = 0.0f, node0[8] = {};
        if (e == hipSuccess) e = hipMemcpyAsync(&root, code, sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(node0, aabb, sizeof(node0), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&notrail, c->d_err + 2, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        t->pairs_root = pt::pairCode(root, leaf_base);
        const float box6[6] = { node0[1], node0[2], node0[3], node0[5], node0[6], node0[7] };
        std::memcpy(t->pairs_root_box, box6, sizeof(box6));
        t->pairs_bytes = (uint32_t)rec_bytes;
        // the restart trail's jump table, for trees it can walk (one parent per node, depth <= 28)
        if (e == hipSuccess && !notrail) {
            e = tpass(3, t->pairs_root);
            if (e == hipSuccess) t->pairs_top = (uint32_t)top_base;
        }
    }
    if (scratch) { hipStreamSynchronize(c->stream); hipFree(scratch); }
    if (e != hipSuccess) { *rc = hipfail(c, e, "BVH child-pair build"); return false; }
    t->pairs_ok = !bad;
    return t->pairs_ok;
}

// launch a deferred order build now, as its own kernel
int flush_order(Dev* c)
{
    if (!c->order_pending) return PT_OK;
    c->order_pending = false;
    HIPCHK(c, pt_launch_order_build(&c->pending_order, c->stream));
    return PT_OK;
}

// A path-tracing draw's arguments from the effect's uniforms and samplers, checked; `mesh`: the program walks a BVH
// (whose child-pair records are built here when its textures changed)
int trace_args(DevFx* fx, DevTex* target, pt::TraceArgs& a, bool& mesh)
{
    Dev* c = fx->ctx;
    if (!target || target->kind != TEX_RT) return fail(c, PT_ERR_ARG, "path tracing draws need a render target");
    DevTex* prev = sampler(fx, "previousBuffer");
    DevTex* bn = sampler(fx, "blueNoiseTexture");
    if (!prev || prev->kind == TEX_U8 || prev->w != target->w || prev->h != target->h)
        return fail(c, PT_ERR_STATE, "previousBuffer must be an RGBA32F texture of the target's size");
    if (!bn || bn->kind != TEX_U8) return fail(c, PT_ERR_STATE, "blueNoiseTexture must be bound (RGBA8)");
    std::memset(&a, 0, sizeof(a));
    a.width = target->w;
    a.height = target->h;
    a.num_parts = c->num_parts;
    a.part = c->part;
    a.res[0] = uf(fx, "uResolution", 0); a.res[1] = uf(fx, "uResolution", 1);
    a.rnd[0] = uf(fx, "uRandomVec2", 0); a.rnd[1] = uf(fx, "uRandomVec2", 1);
    a.ulen = uf(fx, "uULen"); a.vlen = uf(fx, "uVLen");
    a.frame = uf(fx, "uFrameCounter");
    a.eps = uf(fx, "uEPS_intersect");
    a.aperture = uf(fx, "uApertureSize");
    a.focus = uf(fx, "uFocusDistance");
    a.moving = ui(fx, "uCameraIsMoving");
    um4(fx, "uCameraMatrix", a.cam);
    setup_scene(fx, a);
    a.prev = (const float4*)prev->d;
    a.out = (float4*)target->d;
    a.bluenoise = tex8(bn);
    mesh = fx->prog == PT_PROG_GLTF || fx->prog == PT_PROG_HDRI || fx->prog == PT_PROG_SKY_MESH;
    if (mesh) {
        DevTex* bvh = sampler(fx, "tAABBTexture");
        DevTex* tri = sampler(fx, "tTriangleTexture");
        if (!bvh || !tri || bvh->kind != TEX_F32 || tri->kind != TEX_F32)
            return fail(c, PT_ERR_STATE, "tAABBTexture / tTriangleTexture must be bound RGBA32F data textures");
        um4(fx, "uGLTF_Model_InvMatrix", a.model);
        a.model_mat = ui(fx, "uModelMaterialType");
        a.uses_albedo = ui(fx, "uModelUsesAlbedoTexture");
        a.uses_bump = ui(fx, "uModelUsesBumpTexture");
        a.uses_metal = ui(fx, "uModelUsesMetallicTexture");
        a.uses_emissive = ui(fx, "uModelUsesEmissiveTexture");
        a.aabb = (const float4*)bvh->d;
        a.aabb_texels = (long long)bvh->w * bvh->h;
        a.tri = (const float4*)tri->d;
        a.tri_texels = (long long)tri->w * tri->h;
        int prc = PT_OK;
        if (ensure_pairs(c, bvh, tri, &prc)) {
            a.bvh_pairs = bvh->pairs_inner;
            a.bvh_root_code = bvh->pairs_root;
            std::memcpy(a.bvh_root_box, bvh->pairs_root_box, sizeof(a.bvh_root_box));
            a.bvh_pairs_bytes = bvh->pairs_bytes;
            a.bvh_top_base = c->bvh_layout == PT_BVH_TRAIL ? bvh->pairs_top : 0u;
        }
        if (prc) return prc;
        a.bvh_walk = a.bvh_top_base ? pt::WALK_TRAIL : a.bvh_pairs ? pt::WALK_PAIRS : pt::WALK_REF;
        c->bvh_used = a.bvh_top_base ? PT_BVH_TRAIL : a.bvh_pairs ? PT_BVH_PAIRS : PT_BVH_REFERENCE;
        a.albedo = tex8(sampler(fx, "tAlbedoTexture"));
        a.bump = tex8(sampler(fx, "tBumpTexture"));
        a.metal = tex8(sampler(fx, "tMetallicTexture"));
        a.emissive = tex8(sampler(fx, "tEmissiveTexture"));
    }
    a.counters = c->d_counters;
    a.err = c->d_err;
#ifdef PT_SECPROF
    {   // experiment builds: the wave timeline of the last megakernel draw (pt_debug_wave_log)
        static size_t cap = 0;
        const size_t tx = (size_t)((target->w + pt::kTile - 1) / pt::kTile);   // + split tiles' padding rows
        const size_t need = (tx * bands_owned(c, target->h) * 4 + (4 * pt::kSplitParts - 4) * (size_t)c->k.split_tiles + 4 * tx) * pt::kWaveLogSlots;
        if (cap < need) { if (g_wave_log) hipFree(g_wave_log); hipMalloc(&g_wave_log, need * 8); cap = need; }
        hipMemsetAsync(g_wave_log, 0, need * 8, c->stream);   // padding workgroups leave zero rows
        g_wave_log_n = need / pt::kWaveLogSlots;
        a.wave_log = g_wave_log;
        // the walk statistics' global atomics (every wave, every bounce) slow the launch ~4x and skew
        // the timeline by XCD: only when asked for (tools/walkstat.py sets PT_WALKSTAT=1)
        static const bool walkstat = std::getenv("PT_WALKSTAT") && std::atoi(std::getenv("PT_WALKSTAT")) != 0;
        if (walkstat && !g_walk_stat && hipMalloc(&g_walk_stat, 40 * 8) == hipSuccess) hipMemset(g_walk_stat, 0, 40 * 8);
        a.walk_stat = walkstat ? g_walk_stat : nullptr;
    }
#endif
    return PT_OK;
}

// The feature targets of a draw of `target`, checked (pt_set_feature_targets)
int feature_check(const DevFx* fx, const DevTex* target)
{
    Dev* c = fx->ctx;
    const DevTex* prev = sampler(fx, "previousBuffer");
    for (int k = 0; k < 2; k++) {
        const DevTex* t = fx->feat[k];
        if (!t) continue;
        if (t->w != target->w || t->h != target->h)
            return fail(c, PT_ERR_STATE, "a feature target must have the draw target's size");
        if (t == target || t->d == target->d || (prev && (t == prev || t->d == prev->d)))
            return fail(c, PT_ERR_STATE, "a feature target must not be the draw target or previousBuffer");
    }
    if (fx->feat[0] && fx->feat[1] && (fx->feat[0] == fx->feat[1] || fx->feat[0]->d == fx->feat[1]->d))
        return fail(c, PT_ERR_STATE, "the two feature targets must be distinct");
    return PT_OK;
}

// the feature fold of a draw, from the G-buffer staged at g0 / g1 (`stride` pixels per row)
pt::FoldArgs fold_args(const DevFx* fx, const pt::TraceArgs& a, const float4* g0, const float4* g1, int stride)
{
    return pt::FoldArgs{ a.width, a.height, a.num_parts, a.part, a.frame, a.moving, g0, g1, stride,
                         fx->feat[0] ? (float4*)fx->feat[0]->d : nullptr, fx->feat[1] ? (float4*)fx->feat[1]->d : nullptr };
}

// The wavefront / persistent schedules (and a draw that owns no band) over gx x gy tiles: on the main stream,
// their finish pass accumulating; the next megakernel draw waits for all of it (they share the spill slab)
int draw_queued(DevFx* fx, DevTex* target, pt::TraceArgs& a, bool mesh, int gx, int gy)
{
    Dev* c = fx->ctx;
    const int persist = ((c->cu_count * 4 + pt::kShards - 1) / pt::kShards) * pt::kShards;
    if (c->backend == PT_BACKEND_WAVEFRONT) {
        // the quad-rounded frame is what gets shaded (helpers at odd edges included)
        int rc = wf_reserve(c, (target->w + 1) & ~1, (target->h + 1) & ~1, gx * gy, persist);
        if (rc) return rc;
    }
    const unsigned n_wave_tiles = (unsigned)gx * gy * 4u;
    if (c->backend == PT_BACKEND_PERSISTENT) {
        int rc = gb_reserve(c, (target->w + 1) & ~1, (target->h + 1) & ~1);
        if (rc) return rc;
        const unsigned waves = (n_wave_tiles + c->k.persist_tiles - 1) / c->k.persist_tiles;
        const size_t lanes = (size_t)((waves + 3) / 4) * pt::kBlock;
        if (lanes * kSpillPerLane > 0xffffffffull)   // 32-bit slab index
            return fail(c, PT_ERR_ARG, "render target too large for the BVH stack slab");
        if (mesh && (rc = spill_reserve(c, lanes))) return rc;
        a.spill = c->mk_spill;
        a.spill_stride = lanes;
    }
    if (c->backend != PT_BACKEND_MEGAKERNEL) c->ov.need_fresh = true;
    int rc = begin_draw(c, fx->prog);
    if (rc) return rc;
    if (gy > 0 && c->backend == PT_BACKEND_WAVEFRONT) {
        HIPCHK(c, hipMemsetAsync(c->wf.cnt, 0, 16 * pt::kShards * sizeof(unsigned), c->stream));
        HIPCHK(c, pt_launch_wavefront(fx->prog, c->counting ? 1 : 0, &a, &c->wf, gx, gy, persist, c->stream));
    } else if (gy > 0 && c->backend == PT_BACKEND_PERSISTENT) {
        HIPCHK(c, pt_launch_persist(fx->prog, c->counting ? 1 : 0, &a, &c->gb, gx, n_wave_tiles, (unsigned)c->k.persist_tiles,
                                    (unsigned)c->k.persist_refill, c->stream));
        HIPCHK(c, pt_launch_finish(&a, &c->gb, gx, gy, c->stream));
    }
    if (int erc = end_draw(c, fx->prog)) return erc;
    // feature targets: folded from the backend's per-pixel G-buffer (quad-rounded rows), after its finish pass
    if (gy > 0 && c->backend != PT_BACKEND_MEGAKERNEL && (fx->feat[0] || fx->feat[1])) {
        const pt::WfBufs& w = c->backend == PT_BACKEND_WAVEFRONT ? c->wf : c->gb;
        const pt::FoldArgs f = fold_args(fx, a, w.gb0, w.gb1, w.wq);
        HIPCHK(c, pt_launch_feature_fold(&f, gy, c->stream, 0));
    }
    return PT_OK;
}

// The megakernel draw over gx x gy tiles: plan (pt_plan.h), reserve, wait, launch, blend, defer the order build
int draw_mega(DevFx* fx, DevTex* target, pt::TraceArgs& a, bool mesh, int gx, int gy)
{
    Dev* c = fx->ctx;
    // ---- plan. Late-bounce compaction and the frames in flight first (cont_decide).
    // A moving-camera draw that runs alone (PT_MOVING_SERIAL) does not compact: with no next frame beside it,
    // pt_cont's tail (a wave waits for its longest chain of walks) is the frame's (dragon stand-in 1080p
    // 1.19 -> 1.09 ms per frame, profiles/r06af_movpx.log); its slowest tiles are split instead. Nor is it a
    // draw of the auto trial, and pt_queue_stats reports it as not compacting.
    const bool alone = a.moving && c->k.moving_serial;
    pt::ContTrial::Draw trial;
    if (int rc = cont_decide(c, target, fx->prog, mesh && !c->counting && !PT_SECPROF_BUILD, alone, &trial)) return rc;
    const bool cont = trial.on;
    const int depth = trial.depth;
    const size_t share = share_pixels(c, target);
    const int lag = pt::draw_lag(c->k, share);
    const pt::Overlap::Slot at = c->ov.slot(depth, lag);   // draw k = mk_seq: buffer set k % (depth + lag), stream k % depth
    // longest-first: the costs of draw k - sets (same buffer set) order this one if it drew the same thing
    const Dev::LptKey& key = c->lpt_key[at.set];
    const bool lpt = c->k.lpt && !c->counting;
    const bool same = lpt && key.valid && key.n == (size_t)gx * gy && key.target == target && key.prog == fx->prog &&
                      key.part == c->part && key.parts == c->num_parts && c->lpt_cap >= key.n;
    const pt::MegaGrid g(gx, gy, same, cont, c->k);
    // where the path tracing runs: a side stream gated by the main stream's state when an earlier megakernel
    // draw began (or now: the first draw, after another schedule or a stream switch, with counting kernels, or
    // when a sampler is a render target, which draws on the main stream may write)
    bool overlap = c->k.overlap && !c->counting && !PT_SECPROF_BUILD && !alone;   // (experiment builds: one wave log)
    for (const auto& kv : fx->samplers)
        if (kv.second && kv.second->kind == TEX_RT && kv.first != "previousBuffer") overlap = false;

    // ---- reserve (new memory makes the draw wait for everything before it: slab_grow)
    if (mesh) {
        if (g.lanes * kSpillPerLane > 0xffffffffull)   // 32-bit slab index
            return fail(c, PT_ERR_ARG, "render target too large for the BVH stack slab");
        if (int rc = spill_reserve(c, g.lanes)) return rc;
        a.spill = spill_slab(c, at.stream);
        a.spill_stride = g.lanes;
    }
    if (int rc = rad_reserve(c, (size_t)target->w * target->h)) return rc;
    a.rad = c->rad_mem + (size_t)at.set * c->rad_pixels;
    const bool feat = fx->feat[0] || fx->feat[1];
    if (feat) {   // the set's staged G-buffer: two planes
        if (int rc = feat_reserve(c, (size_t)target->w * target->h)) return rc;
        a.feat0 = c->feat_mem + (size_t)at.set * 2 * c->feat_pixels;
        a.feat1 = a.feat0 + c->feat_pixels;
    }
    if (cont) {   // (records for this draw's set: allocated by cont_decide already, unless the lag changed)
        if (int rc = cont_reserve(c, owned_pixels(c, target), depth + lag)) return rc;
        // (the record sort's keys take the model's root box: child-pair walks only)
        cont_args(c, at.set, c->k.cont_sort && a.bvh_walk != pt::WALK_REF, a);
    }
    if (lpt && c->lpt_cap < g.n) {   // cost | order | split; pt_trace on the side streams reads the order and writes the costs
        if (int rc = slab_grow(c, c->lpt_mem, c->lpt_cap, g.n, (5 * g.n + 1) * Dev::kSetsMax * sizeof(unsigned), WAIT_ALL, true))
            return rc;
        for (auto& k : c->lpt_key) k.valid = false;
    }

    // ---- wait: the main stream's mark for this draw, and the mark pt::Overlap picks for its path tracing
    hipStream_t ts = c->stream;
    if (overlap)
        if (int rc = overlap_init(c)) return rc;
    const int wait = c->ov.step(depth, lag, overlap).wait;
    if (overlap) {
        HIPCHK(c, hipEventRecord(c->ev_mark[at.set], c->stream));
        ts = c->ts[at.stream];
        HIPCHK(c, hipStreamWaitEvent(ts, c->ev_mark[wait], 0));
    }

    // ---- launch, on `ts`
    if (lpt) {
        if (!same) HIPCHK(c, hipMemsetAsync(c->lpt_cost(at.set), 0, 4 * g.n * sizeof(unsigned), ts));   // costs start afresh
        a.order = same ? c->lpt_order(at.set) : nullptr;
        a.cost = c->lpt_cost(at.set);
        a.order_zig = g.order_zig;
        a.split = (a.order && g.split) ? c->lpt_split(at.set) : nullptr;
    }
    a.ntiles = (unsigned)g.n;
    if (int rc = begin_draw(c, fx->prog, ts)) return rc;
    if (a.cont_bins) {   // (PT_CONT_SORT) the key's origin cells over the model's root box
        a.cont_grid_bits = pt::MegaGrid::sort_grid_bits(c->k, share);
        for (int k = 0; k < 3; k++) {
            const float ext = a.bvh_root_box[3 + k] - a.bvh_root_box[k];
            a.cont_cell[k] = ext > 0.0f ? (float)(1u << a.cont_grid_bits) / ext : 0.0f;
        }
    }
    HIPCHK(c, pt_launch_trace(fx->prog, c->counting ? 1 : 0, &a, gx, a.split ? g.gy_grid : gy, ts));
    if (a.cont_bins) {   // ... and the records' order, from the keys' totals and ranks pt_trace took
        pt::SortArgs so;
        std::memset(&so, 0, sizeof(so));
        so.count = a.cont_count;
        so.key = a.cont_key;
        so.rank = a.cont_rank;
        so.bins = a.cont_bins;
        so.perm = (unsigned*)a.cont_perm;
        so.nbins = 16u << (3u * a.cont_grid_bits);
        HIPCHK(c, pt_launch_cont_sort(&so, c->cont_cap, ts));
    }
    if (cont) {   // (its one-wave workgroups index the spill slab below the trace grid's lanes)
        HIPCHK(c, pt_launch_cont(fx->prog, &a, g.cont_waves(c->k, share, fx->prog == PT_PROG_SKY_MESH), ts));
        c->cont_draws++;
    }
    // the draw's timing events bracket all of its path tracing on the side stream: pt_trace and, when the
    // draw compacts, pt_cont (the blend below is the main stream's)
    if (int rc = end_draw(c, fx->prog, ts)) return rc;
    if (overlap) {
        HIPCHK(c, hipEventRecord(c->ev_traced[at.stream], ts));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_traced[at.stream], 0));
    }

    // ---- blend: the history half of main() on the main stream, where the copy / output draws that read the
    // accumulation follow
    pt::BlendArgs b{ a.width, a.height, a.num_parts, a.part, a.frame, a.moving, a.rad, a.prev, a.out, a.cont_count, a.cont_bins };
    HIPCHK(c, pt_launch_blend(&b, gy, c->stream, g.one_wave ? c->k.main_waves : 0));
    // ---- feature targets: the staged G-buffer folded right after, on the main stream too, so folds keep the draws' order
    if (feat) {
        const pt::FoldArgs f = fold_args(fx, a, a.feat0, a.feat1, a.width);
        HIPCHK(c, pt_launch_feature_fold(&f, gy, c->stream, g.one_wave ? c->k.main_waves : 0));
    }

    // ---- this draw's costs order draw k + sets: the build rides along with the next screenOutput
    if (a.cost) {
        c->pending_order = { (unsigned)g.n, a.cost, c->lpt_order(at.set), c->lpt_split(at.set), g.split_cap,
                             (unsigned)c->k.split_dominance, c->k.split_near, c->k.lpt_flat, (unsigned)c->k.lpt_flat_tiles };
        c->order_pending = true;
        if (!c->k.fuse_order) { if (int rc = flush_order(c)) return rc; }
        c->lpt_key[at.set] = { true, g.n, target, fx->prog, c->part, c->num_parts };
    }
    c->ov.mk_seq++;
    return PT_OK;
}

int render_trace(DevFx* fx, DevTex* target)
{
    Dev* c = fx->ctx;
    if (int rc = flush_order(c)) return rc;   // the last draw's order (before lpt_mem could be reallocated)
    pt::TraceArgs a;
    bool mesh = false;
    if (int rc = trace_args(fx, target, a, mesh)) return rc;
    if (int rc = feature_check(fx, target)) return rc;
    const int gx = (target->w + pt::kTile - 1) / pt::kTile, gy = bands_owned(c, target->h);
    return c->backend == PT_BACKEND_MEGAKERNEL && gy > 0 ? draw_mega(fx, target, a, mesh, gx, gy)
                                                         : draw_queued(fx, target, a, mesh, gx, gy);
}

int launch_copy(Dev* c, DevTex* src, DevTex* dst, int num_parts, int part)
{
    pt::CopyArgs a{ dst->w, dst->h, num_parts, part, (const float4*)src->d, (float4*)dst->d };
    const int gx = (dst->w + 255) / 256, gy = pt::bands_owned(dst->h, num_parts, part);
    if (gy > 0) HIPCHK(c, pt_launch_copy(&a, gx, gy, c->stream));
    return PT_OK;
}

// run a deferred screenCopy now, as its own kernel (timed as a screenCopy draw)
int flush_copy(Dev* c)
{
    if (!c->pending_copy.on) return PT_OK;
    c->pending_copy.on = false;
    int rc = begin_draw(c, PT_PROG_SCREEN_COPY);
    if (rc) return rc;
    rc = launch_copy(c, c->pending_copy.src, c->pending_copy.dst, c->pending_copy.num_parts, c->pending_copy.part);
    if (rc) return rc;
    return end_draw(c, PT_PROG_SCREEN_COPY);
}

int render_copy(DevFx* fx, DevTex* target)
{
    Dev* c = fx->ctx;
    DevTex* src = sampler(fx, "pathTracedImageBuffer");
    if (!target || target->kind != TEX_RT) return fail(c, PT_ERR_ARG, "screenCopy needs a render target");
    if (!src || src->kind == TEX_U8 || src->w != target->w || src->h != target->h)
        return fail(c, PT_ERR_STATE, "pathTracedImageBuffer must be an RGBA32F texture of the target's size");
    int rc = flush_copy(c);
    if (rc) return rc;
    // deferred: the render loop's next draw is screenOutput of the same source, which writes the
    // copy target in the same pass (render_output); any other use flushes it first (flush_copy)
    if (src != target) c->pending_copy = { true, src, target, c->num_parts, c->part };
    return PT_OK;
}

int render_output(DevFx* fx, DevTex* target)
{
    Dev* c = fx->ctx;
    DevTex* acc = sampler(fx, "accumulationBuffer");
    if (!acc || acc->kind == TEX_U8) return fail(c, PT_ERR_STATE, "accumulationBuffer must be an RGBA32F texture");
    pt::OutputArgs a;
    std::memset(&a, 0, sizeof(a));
    a.acc = (const float4*)acc->d;
    a.acc_w = acc->w;
    a.acc_h = acc->h;
    a.one_over_n = uf(fx, "uOneOverSampleCounter");
    a.exposure = uf(fx, "uToneMappingExposure");
    a.num_parts = c->output_partition ? c->num_parts : 1;
    a.part = c->output_partition ? c->part : 0;
    // fuse the deferred screenCopy when this pass covers exactly its texels: same source, same
    // frame size, same bands, and the copy target is not this pass's output
    const auto& pc = c->pending_copy;
    const int ow = target ? target->w : (c->cw || c->ch ? c->cw : acc->w), oh = target ? target->h : (c->cw || c->ch ? c->ch : acc->h);
    const bool fuse = pc.on && pc.src == acc && pc.dst != target && ow == acc->w && oh == acc->h &&
                      pc.num_parts == a.num_parts && (pc.num_parts == 1 || pc.part == a.part);
    if (fuse) { a.copy_dst = (float4*)pc.dst->d; c->pending_copy.on = false; }
    else { int frc = flush_copy(c); if (frc) return frc; }
    if (target) {
        if (target->kind != TEX_RT) return fail(c, PT_ERR_ARG, "screenOutput target must be a render target or the canvas");
        a.width = target->w; a.height = target->h; a.out_f = (float4*)target->d;
    } else {
        if (c->cw == 0 && c->ch == 0) {
            int rc = dev_canvas_resize(c, acc->w, acc->h);
            if (rc) return rc;
        }
        a.width = c->cw; a.height = c->ch; a.canvas = c->canvas;
    }
    // the order build rides along only up to 32768 tiles (4K): beyond, the block's 256 threads would
    // loop over memory and outlast the pass, so it runs alone first (1024 threads)
    if (c->order_pending && c->pending_order.ntiles > pt::kOrderHeld * 256u)
        if (int frc = flush_order(c)) return frc;
    int rc = begin_draw(c, fx->prog);
    if (rc) return rc;
    if (a.width > 0 && a.height > 0) {
        if (c->order_pending) {   // the last megakernel draw's order build rides along as one more block
            a.ob = c->pending_order;
            c->order_pending = false;
        }
        // one-wave workgroups while a fused order build fits one wave's registers (<= 8192 tiles: up to
        // ~2 MP, and a rank's share of 4K), else the 4-wave blocks with a 256-thread order build
        const unsigned tiles = (unsigned)((a.width + 15) / 16) * (unsigned)pt::bands_owned(a.height, a.num_parts, a.part);   // (as pt_launch_output's grid)
        const bool one = std::max(tiles, a.ob.ntiles) <= pt::kOrderHeld * 64u;   // (ob.ntiles 0: no order build)
        HIPCHK(c, pt_launch_output(&a, c->stream, one ? c->k.main_waves : 0));
    }
    return end_draw(c, fx->prog);
}

DevTex* new_texture(Dev* c, int kind, int w, int h, size_t texel, int* err)
{
    auto* t = new DevTex();
    t->ctx = c; t->kind = kind; t->w = w; t->h = h;
    t->bytes = (size_t)w * (size_t)h * texel;
    if (t->bytes) {
        hipError_t e = hipMalloc(&t->d, t->bytes);
        if (e != hipSuccess) {
            hipfail(c, e, "hipMalloc");
            delete t;
            if (err) *err = PT_ERR_OOM;
            return nullptr;
        }
    }
    c->textures.insert(t);
    return t;
}

DevTex* upload(Dev* c, int kind, int w, int h, const void* data, size_t texel, int sampling, int invert_y, int* err)
{
    if (err) *err = PT_OK;
    if (!c || w <= 0 || h <= 0 || (long long)w * h >= (1ll << 31)) { if (err) *err = PT_ERR_ARG; return nullptr; }
    hipSetDevice(c->device);
    DevTex* t = new_texture(c, kind, w, h, texel, err);
    if (!t) return nullptr;
    t->sampling = sampling; t->invert_y = invert_y;
    hipError_t e = hipSuccess;
    if (!data) e = hipMemsetAsync(t->d, 0, t->bytes, c->stream);
    else if (!invert_y) e = hipMemcpyAsync(t->d, data, t->bytes, hipMemcpyHostToDevice, c->stream);
    else {
        const size_t row = (size_t)w * texel;   // UNPACK_FLIP_Y: source row r lands on row h-1-r
        for (int r = 0; r < h && e == hipSuccess; r++)
            e = hipMemcpyAsync((char*)t->d + (size_t)(h - 1 - r) * row, (const char*)data + (size_t)r * row, row,
                               hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the caller keeps ownership of data
    if (e != hipSuccess) {
        hipfail(c, e, "texture upload");
        dev_texture_destroy(t);
        if (err) *err = PT_ERR_HIP;
        return nullptr;
    }
    return t;
}

}  // namespace

// ---------------------------------------------------------------------------- device-level API
// (pt_dev.h; the exported C ABI in pt_group.cpp forwards here, once per part of a context)

Dev* dev_ctx_create(int device, int* err)
{
    if (err) *err = PT_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        if (err) *err = PT_ERR_DEVICE;
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        if (err) *err = PT_ERR_DEVICE;   // the code objects are gfx950-only
        return nullptr;
    }
    auto* c = new Dev();
    c->device = device;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    pt::read_knobs(c->k);
    c->ov.depth_run = c->k.depth;
    c->bvh_layout = c->k.bvh_layout;
    c->draw_events = c->k.draw_events != 0;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    c->stream = c->own_stream;
    if (e == hipSuccess) e = hipMalloc(&c->d_err, 256);
    if (e == hipSuccess) e = hipMalloc(&c->d_counters, pt::C_NUM * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(c->d_err, 0, 256, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_counters, 0, pt::C_NUM * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (err) *err = PT_ERR_HIP;
        dev_ctx_destroy(c);
        return nullptr;
    }
    return c;
}

void dev_ctx_destroy(Dev* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    c->pending_copy.on = false;   // nothing can observe its target any more
    c->order_pending = false;     // ... nor a next draw the order
    if (c->stream) hipStreamSynchronize(c->stream);
    for (int p = 0; p < Dev::kDepthMax; p++)   // (pt_trace on the side streams reads and writes the order arrays)
        if (c->ts[p]) hipStreamSynchronize(c->ts[p]);
    std::vector<DevFx*> fx(c->effects.begin(), c->effects.end());
    for (auto* f : fx) dev_effect_destroy(f);
    std::vector<DevTex*> tx(c->textures.begin(), c->textures.end());
    for (auto* t : tx) dev_texture_destroy(t);
    for (auto& pr : c->pool) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (int i = 0; i < kProgSlots; i++) {
        if (c->ev0[i]) hipEventDestroy(c->ev0[i]);
        if (c->ev1[i]) hipEventDestroy(c->ev1[i]);
    }
    if (c->canvas && !c->canvas_external) hipFree(c->canvas);
    if (c->wf_mem) hipFree(c->wf_mem);
    if (c->lpt_mem) hipFree(c->lpt_mem);
    if (c->mk_spill) hipFree(c->mk_spill);
    if (c->rad_mem) hipFree(c->rad_mem);
    if (c->feat_mem) hipFree(c->feat_mem);
    if (c->cont_mem) hipFree(c->cont_mem);
    for (auto& e : c->tune_ev) if (e) hipEventDestroy(e);
    for (int p = 0; p < Dev::kSetsMax; p++)
        if (c->ev_mark[p]) hipEventDestroy(c->ev_mark[p]);
    for (int p = 0; p < Dev::kDepthMax; p++) {   // (every side-stream draw was waited for by a blend on the main stream)
        if (c->ts[p]) { hipStreamSynchronize(c->ts[p]); hipStreamDestroy(c->ts[p]); }
        if (c->ev_traced[p]) hipEventDestroy(c->ev_traced[p]);
    }
    if (c->gb_mem) hipFree(c->gb_mem);
    if (c->d_err) hipFree(c->d_err);
    if (c->d_counters) hipFree(c->d_counters);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

const char* dev_last_error(Dev* c) { return c ? c->err.c_str() : "no context"; }

int dev_sync(Dev* c)
{
    if (!c) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned flags = 0;
    HIPCHK(c, hipMemcpy(&flags, c->d_err, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags) {   // (on the main stream, which the next draw's path tracing waits for: not the null stream)
        HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(unsigned), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ov.need_fresh = true;
        if (flags & pt::E_STACK) return fail(c, PT_ERR_DATA, "BVH traversal needed more than stackLevels[28]");
    }
    return PT_OK;
}

int dev_canvas_resize(Dev* c, int w, int h)
{
    if (!c || w < 0 || h < 0) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (w == c->cw && h == c->ch && c->canvas && !c->canvas_external) return PT_OK;
    if (c->canvas) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!c->canvas_external) HIPCHK(c, hipFree(c->canvas));
        c->canvas = nullptr;
    }
    c->canvas_external = false;
    c->cw = w; c->ch = h;
    if (w * (size_t)h) {
        HIPCHK(c, hipMalloc(&c->canvas, (size_t)w * h * sizeof(uchar4)));
        HIPCHK(c, hipMemsetAsync(c->canvas, 0, (size_t)w * h * sizeof(uchar4), c->stream));
    }
    return PT_OK;
}

int dev_canvas_wrap(Dev* c, int w, int h, void* ptr)
{
    if (!c || w <= 0 || h <= 0 || !ptr) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->canvas && !c->canvas_external) {   // switching between wrapped canvases needs no sync
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(c->canvas));
    }
    c->canvas = (uchar4*)ptr;
    c->canvas_external = true;
    c->cw = w; c->ch = h;
    return PT_OK;
}

int dev_set_output_partition(Dev* c, int enable)
{
    if (!c) return PT_ERR_ARG;
    c->output_partition = enable != 0;
    return PT_OK;
}

DevFx* dev_effect_create(Dev* c, const char* src, const char* const* un, int nu, const char* const* sn, int ns, int* err)
{
    if (err) *err = PT_OK;
    if (!c || !src) { if (err) *err = PT_ERR_ARG; return nullptr; }
    int prog = classify(src);
    if (prog == PT_PROG_UNKNOWN) {
        fail(c, PT_ERR_SHADER, "fragment shader not recognised as a reference path-tracing program");
        if (err) *err = PT_ERR_SHADER;
        return nullptr;
    }
    return dev_effect_create_program(c, prog, un, nu, sn, ns, err);
}

DevFx* dev_effect_create_program(Dev* c, int prog, const char* const* un, int nu, const char* const* sn, int ns, int* err)
{
    if (err) *err = PT_OK;
    if (!c || nu < 0 || ns < 0 || prog <= PT_PROG_UNKNOWN || prog > PT_PROG_SKY_MESH) { if (err) *err = PT_ERR_ARG; return nullptr; }
    auto* fx = new DevFx();
    fx->ctx = c;
    fx->prog = prog;
    for (int i = 0; i < nu; i++) if (un && un[i]) fx->uniforms[un[i]] = Uniform();
    for (int i = 0; i < ns; i++) if (sn && sn[i]) fx->samplers[sn[i]] = nullptr;
    c->effects.insert(fx);
    return fx;
}

void dev_effect_destroy(DevFx* fx)
{
    if (!fx) return;
    fx->ctx->effects.erase(fx);
    delete fx;
}

int dev_effect_program(const DevFx* fx) { return fx ? fx->prog : PT_PROG_UNKNOWN; }

int dev_set_float(DevFx* fx, const char* name, const float* v, int n)
{
    if (!fx || !name || !v || n < 1 || n > 16) return PT_ERR_ARG;
    auto it = fx->uniforms.find(name);
    if (it == fx->uniforms.end()) return PT_OK;   // undeclared: ignored, as in Babylon
    Uniform& u = it->second;
    u.is_int = false; u.n = n; u.set = true;
    for (int k = 0; k < n; k++) u.f[k] = v[k];
    return PT_OK;
}

int dev_set_int(DevFx* fx, const char* name, int v)
{
    if (!fx || !name) return PT_ERR_ARG;
    auto it = fx->uniforms.find(name);
    if (it == fx->uniforms.end()) return PT_OK;
    Uniform& u = it->second;
    u.is_int = true; u.n = 1; u.i = v; u.set = true;
    return PT_OK;
}

int dev_set_texture(DevFx* fx, const char* name, DevTex* t)
{
    if (!fx || !name) return PT_ERR_ARG;
    if (t && t->ctx != fx->ctx) return fail(fx->ctx, PT_ERR_ARG, "texture belongs to another context");
    auto it = fx->samplers.find(name);
    if (it == fx->samplers.end()) return PT_OK;
    it->second = t;
    return PT_OK;
}

DevTex* dev_texture_create_rgba32f(Dev* c, int w, int h, const float* data, int sampling, int invert_y, int* err)
{
    return upload(c, TEX_F32, w, h, data, 16, sampling, invert_y, err);
}

DevTex* dev_texture_create_rgba8(Dev* c, int w, int h, const uint8_t* data, int sampling, int invert_y, int* err)
{
    return upload(c, TEX_U8, w, h, data, 4, sampling, invert_y, err);
}

DevTex* dev_render_target_create(Dev* c, int w, int h, int* err)
{
    return upload(c, TEX_RT, w, h, nullptr, 16, PT_SAMPLING_NEAREST, 0, err);
}

DevTex* dev_render_target_wrap(Dev* c, int w, int h, void* dptr, int* err)
{
    if (err) *err = PT_OK;
    if (!c || w <= 0 || h <= 0 || !dptr) { if (err) *err = PT_ERR_ARG; return nullptr; }
    auto* t = new DevTex();
    t->ctx = c; t->kind = TEX_RT; t->w = w; t->h = h;
    t->bytes = (size_t)w * h * 16;
    t->d = dptr;
    t->external = true;
    c->textures.insert(t);
    return t;
}

int dev_render_target_resize(DevTex* t, int w, int h)
{
    if (!t || t->kind != TEX_RT || w <= 0 || h <= 0) return PT_ERR_ARG;
    if (t->external) return fail(t->ctx, PT_ERR_ARG, "wrapped render targets are not resizable");
    Dev* c = t->ctx;
    if (w == t->w && h == t->h) return PT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (t->d) HIPCHK(c, hipFree(t->d));
    t->d = nullptr;
    t->w = w; t->h = h; t->bytes = (size_t)w * h * 16;
    HIPCHK(c, hipMalloc(&t->d, t->bytes));
    HIPCHK(c, hipMemsetAsync(t->d, 0, t->bytes, c->stream));
    return PT_OK;
}

int dev_texture_size(const DevTex* t, int* w, int* h)
{
    if (!t) return PT_ERR_ARG;
    if (w) *w = t->w;
    if (h) *h = t->h;
    return PT_OK;
}

void dev_texture_destroy(DevTex* t)
{
    if (!t) return;
    Dev* c = t->ctx;
    hipSetDevice(c->device);
    if (c->pending_copy.on && (c->pending_copy.src == t || c->pending_copy.dst == t)) flush_copy(c);
    for (auto* fx : c->effects)
        for (auto& kv : fx->samplers)
            if (kv.second == t) kv.second = nullptr;
    for (auto* fx : c->effects)   // a bound feature target: unbound (the folds queued so far are waited for below)
        for (auto& f : fx->feat)
            if (f == t) f = nullptr;
    if (t->d && !t->external) { hipStreamSynchronize(c->stream); hipFree(t->d); }
    if (t->pairs_mem) { hipStreamSynchronize(c->stream); hipFree(t->pairs_mem); }
    for (auto* o : c->textures)   // records built against this triangle texture are stale
        if (o->pairs_tri == t) { o->pairs_tri = nullptr; o->pairs_gen = ~0ull; }
    c->textures.erase(t);
    delete t;
}

int dev_render(DevFx* fx, DevTex* target)
{
    if (!fx) return PT_ERR_ARG;
    Dev* c = fx->ctx;
    if (target && target->ctx != c) return fail(c, PT_ERR_ARG, "target belongs to another context");
    HIPCHK(c, hipSetDevice(c->device));
    if (fx->prog != PT_PROG_SCREEN_OUTPUT && fx->prog != PT_PROG_SCREEN_COPY) {
        int rc = flush_copy(c);
        if (rc) return rc;
    }
    switch (fx->prog) {
    case PT_PROG_CORNELL:
    case PT_PROG_QUADRIC:
    case PT_PROG_SKY:
    case PT_PROG_SKY_MESH:
    case PT_PROG_HDRI:
    case PT_PROG_GLTF: return render_trace(fx, target);
    case PT_PROG_SCREEN_COPY: return render_copy(fx, target);
    case PT_PROG_SCREEN_OUTPUT: return render_output(fx, target);
    default: return fail(c, PT_ERR_UNSUPPORTED, "program recognised but not implemented in this build");
    }
}

int dev_read_pixels(Dev* c, const DevTex* t, void* dst, size_t bytes)
{
    if (!c || !dst) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    const void* src = t ? t->d : (const void*)c->canvas;
    size_t need = t ? t->bytes : (size_t)c->cw * c->ch * sizeof(uchar4);
    if (bytes < need) return fail(c, PT_ERR_ARG, "destination too small");
    HIPCHK(c, hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int dev_write_pixels(Dev* c, DevTex* t, const void* src, size_t bytes)
{
    if (!c || !t || !src || bytes != t->bytes) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(t->d, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->gen++;
    return PT_OK;
}

int dev_set_stream(Dev* c, void* stream)
{
    if (!c) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    if (int rc = flush_order(c)) return rc;        // on the stream its draw ran on
    HIPCHK(c, hipStreamSynchronize(c->stream));   // work already queued finishes first
    c->stream = stream ? (hipStream_t)stream : c->own_stream;
    c->ov.need_fresh = true;   // the next megakernel draw waits for the new stream's state
    return PT_OK;
}

int dev_set_backend(Dev* c, int backend)
{
    if (!c || (backend != PT_BACKEND_MEGAKERNEL && backend != PT_BACKEND_WAVEFRONT && backend != PT_BACKEND_PERSISTENT))
        return PT_ERR_ARG;
    c->backend = backend;
    return PT_OK;
}

int dev_set_bvh_layout(Dev* c, int layout)
{
    if (!c || layout < PT_BVH_REFERENCE || layout > PT_BVH_TRAIL) return PT_ERR_ARG;
    c->bvh_layout = layout;
    return PT_OK;
}

int dev_bvh_layout_used(Dev* c) { return c ? c->bvh_used : PT_ERR_ARG; }

int dev_set_row_partition(Dev* c, int num_parts, int part)
{
    if (!c || num_parts < 1 || part < 0 || part >= num_parts) return PT_ERR_ARG;
    c->num_parts = num_parts;
    c->part = part;
    return PT_OK;
}

void* dev_texture_device_ptr(DevTex* t) { return t ? t->d : nullptr; }

int dev_last_render_ms(Dev* c, int prog, float* ms)
{
    if (!c || !ms || prog < 0 || prog >= kProgSlots) return PT_ERR_ARG;
    if (!c->draw_events) {   // the first call turns the per-draw events on; later draws report
        c->draw_events = true;
        return fail(c, PT_ERR_ARG, "per-draw timing was off: it is on from now, for the next draws");
    }
    if (!c->ev_used[prog]) return fail(c, PT_ERR_ARG, "no timed draw of this program yet");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0[prog], c->ev1[prog]));
    return PT_OK;
}

int dev_timing_begin(Dev* c)
{
    if (!c) return PT_ERR_ARG;
    c->window = true;
    c->window_draws.clear();
    std::fill(c->window_seen, c->window_seen + kProgSlots, 0);
    c->timing_every = pt::knob_timing_every(c->timing_every);
    return PT_OK;
}

int dev_timing_end(Dev* c, int prog, double* total_ms, int* launches)
{
    if (!c || !total_ms || !launches) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->window = false;   // the window is closed; its draws stay readable by further dev_timing_end calls
    double t = 0.0;
    int n = 0;
    for (auto& d : c->window_draws) {
        if (d.first != prog) continue;
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->pool[d.second].first, c->pool[d.second].second));
        t += ms;
        n++;
    }
    *total_ms = t;
    *launches = n;
    return PT_OK;
}

int dev_timing_latency(Dev* c, int prog, float* ms, int cap, int* n)
{
    if (!c || !n || cap < 0 || (cap && !ms)) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_copy(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->window = false;
    // each bracketed draw of `prog` with the next bracketed screenOutput draw: the same frame's, as long as
    // every frame draws one of each (the window brackets every timing_every-th draw of each kind)
    int k = 0, open = -1;
    for (auto& d : c->window_draws) {
        if (d.first == prog) open = d.second;
        else if (d.first == PT_PROG_SCREEN_OUTPUT && open >= 0) {
            float t = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&t, c->pool[open].first, c->pool[d.second].second));
            if (k < cap) ms[k] = t;
            k++;
            open = -1;
        }
    }
    *n = std::min(k, cap);
    return PT_OK;
}

int dev_set_counting(Dev* c, int enable)
{
    if (!c) return PT_ERR_ARG;
    c->counting = enable != 0;
    return PT_OK;
}

int dev_read_counters(Dev* c, uint64_t out[PT_NUM_COUNTERS])
{
    if (!c || !out) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_counters, pt::C_NUM * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

int dev_reset_counters(Dev* c)
{
    if (!c) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->d_counters, 0, pt::C_NUM * sizeof(unsigned long long), c->stream));
    return PT_OK;
}

int dev_queue_stats(Dev* c, uint32_t out[16])
{
    if (!c || !out) return PT_ERR_ARG;
    std::memset(out, 0, 16 * sizeof(uint32_t));
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = flush_order(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int p = c->ov.next().set;   // the tiles the next megakernel draw of the same grid splits
    if (c->lpt_mem && c->lpt_key[p].valid)
        HIPCHK(c, hipMemcpy(&out[7], c->lpt_split(p), sizeof(uint32_t), hipMemcpyDeviceToHost));
    // late-bounce compaction of the last megakernel draw: 0 off, 1 auto decided off, 2 auto decided on,
    // 3 forced on (PT_CONT=1), 4 auto trial, 5 / 6 default on / off; bits 8-15: its frames in flight;
    // bits 16-31: the draws that launched pt_cont so far (mod 2^16);
    // out[15]: the auto trial's ms with it on per ms without (the faster depth), x 1000
    out[14] = (uint32_t)c->cont_last | (uint32_t)c->ov.depth_run << 8 | (c->cont_draws & 0xffffu) << 16;
    const float off = std::min(c->trial.ms_off, c->trial.ms_off2);
    out[15] = (c->cont_last == 1 || c->cont_last == 2) && off > 0.0f ? (uint32_t)(1000.0f * c->trial.ms_on / off) : 0u;
    if (!c->wf_mem) return PT_OK;
    std::vector<unsigned> h(16 * pt::kShards);
    HIPCHK(c, hipMemcpy(h.data(), c->wf.cnt, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int b = 0; b < 7; b++)
        for (int s = 0; s < pt::kShards; s++) {
            out[b] += h[b * pt::kShards + s];
            if (b < 6) out[8 + b] += h[(8 + b) * pt::kShards + s];
        }
    return PT_OK;
}

int dev_cont_stats(Dev* c, uint64_t out[2])
{
    if (!c || !out) return PT_ERR_ARG;
    out[0] = out[1] = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (every draw's pt_blend, which keeps the totals, is on it)
    uint64_t stored = 0;
    if (int rc = cont_totals(c, &stored)) return rc;
    out[0] = c->cont_stored + stored;
    out[1] = c->cont_draws;
    return PT_OK;
}

int dev_set_feature_targets(DevFx* fx, DevTex* normal_id, DevTex* albedo_weight)
{
    if (!fx) return PT_ERR_ARG;
    Dev* c = fx->ctx;
    if (fx->prog == PT_PROG_SCREEN_COPY || fx->prog == PT_PROG_SCREEN_OUTPUT)
        return fail(c, PT_ERR_ARG, "feature targets need a path-tracing effect");
    for (DevTex* t : { normal_id, albedo_weight })
        if (t && (t->ctx != c || t->kind != TEX_RT))
            return fail(c, PT_ERR_ARG, "a feature target must be a render target of this context");
    fx->feat[0] = normal_id;
    fx->feat[1] = albedo_weight;
    return PT_OK;
}

int dev_math_exhaustive(Dev* c, int op, uint64_t* mismatches)
{
    if (!c || !mismatches || op < 0 || op > 1) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    HIPCHK(c, hipMalloc(&d, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, pt_launch_exhaustive(op, d, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long h = 0;
    HIPCHK(c, hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost));
    hipFree(d);
    *mismatches = h;
    return PT_OK;
}

int dev_math_probe(Dev* c, int op, const float* x, const float* y, float* out, int n)
{
    if (!c || !x || !out || n <= 0) return PT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    size_t b = (size_t)n * sizeof(float);
    HIPCHK(c, hipMalloc(&dx, b));
    HIPCHK(c, hipMalloc(&dout, b));
    if (y) HIPCHK(c, hipMalloc(&dy, b));
    HIPCHK(c, hipMemcpy(dx, x, b, hipMemcpyHostToDevice));
    if (y) HIPCHK(c, hipMemcpy(dy, y, b, hipMemcpyHostToDevice));
    HIPCHK(c, pt_launch_math_probe(op, dx, dy, dout, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dout, b, hipMemcpyDeviceToHost));
    hipFree(dx); hipFree(dout);
    if (dy) hipFree(dy);
    return PT_OK;
}


int dev_device(const Dev* c) { return c->device; }
hipStream_t dev_stream(const Dev* c) { return c->stream; }
void* dev_canvas_ptr(Dev* c) { return c->canvas; }
int dev_flush(Dev* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    return flush_copy(c);
}
