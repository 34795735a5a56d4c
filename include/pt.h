/* include/pt.h — C ABI of libpt.so, the MI355X (gfx950) backend behind the Babylon.js effect API.
 *
 * The reference drives its hot path only through Babylon's effect API (js/babylon.js, vendored
 * 5.0.0-alpha.43). Each entry point below is what a binding of that API needs; the comment on
 * each names the reference call it replaces (file:line in the reference repository). A Node
 * N-API addon (babylon.js-pathtracing-renderer_amd/napi/pt_napi.c) binds these for the
 * unmodified setup scripts; ctypes binds them for tests and bench.py.
 *
 * Conventions: plain pointers and sizes; every call returns PT_OK (0) or a negative pt_status
 * and never throws. Device memory is owned by the context. Host arrays are copied at the call.
 * All work of a context is ordered on one HIP stream (the context's own, or the caller's: pt_set_stream);
 * pt_render is asynchronous and pt_read_pixels / pt_sync synchronise. The megakernel's path tracing of a
 * frame runs on one of the context's internal side streams (two or three, PT_OVERLAP_DEPTH) beside the
 * previous frames' (frame overlap: it never reads the history), gated by events recorded on the
 * context's stream, and the history blend that follows it runs on that one stream, so every observable
 * result is in call order. Not re-entrant (single JS thread, like the reference).
 * Image rows are stored bottom-up (row 0 = gl_FragCoord.y 0.5), as GL render targets are.
 */
#ifndef PT_H
#define PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_ctx pt_ctx;
typedef struct pt_effect pt_effect;
typedef struct pt_texture pt_texture;

enum pt_status {
    PT_OK = 0,
    PT_ERR_ARG = -1,         /* bad handle, size or name */
    PT_ERR_HIP = -2,         /* HIP runtime error (message in pt_last_error) */
    PT_ERR_SHADER = -3,      /* fragment source not recognised as a supported program */
    PT_ERR_STATE = -4,       /* e.g. render with a required sampler unbound */
    PT_ERR_OOM = -5,
    PT_ERR_DEVICE = -6,      /* no usable gfx950 device */
    PT_ERR_UNSUPPORTED = -7, /* recognised program that this build does not implement yet */
    PT_ERR_DATA = -8         /* scene data outside the reference's limits (e.g. BVH deeper than stackLevels[28]) */
};

/* Programs recognised from the fragment source registered in Effect.ShadersStore. */
enum pt_program {
    PT_PROG_UNKNOWN = 0,
    PT_PROG_SCREEN_COPY = 1,    /* js/PathTracingCommon.js:1-16 */
    PT_PROG_SCREEN_OUTPUT = 2,  /* js/PathTracingCommon.js:19-309 */
    PT_PROG_CORNELL = 3,        /* js/BabylonPathTracing_FragmentShader.js */
    PT_PROG_GLTF = 4,           /* js/GLTFModelPathTracing_FragmentShader.js */
    PT_PROG_HDRI = 5,           /* js/HDRIEnvironmentPathTracing_FragmentShader.js */
    PT_PROG_SKY = 6,            /* js/PhysicalSkyModel_FragmentShader.js */
    PT_PROG_QUADRIC = 7,        /* js/TransformedQuadricGeometry_FragmentShader.js */
    /* BASELINE configs[4]: js/PhysicalSkyModel_FragmentShader.js with the glTF model block of
     * js/GLTFModelPathTracing_FragmentShader.js:201-346 appended to its SceneIntersect (the sky shader
     * text plus `uniform sampler2D tAABBTexture`); the reference has no such page */
    PT_PROG_SKY_MESH = 8
};

/* Babylon sampling-mode constants (BABYLON.Constants.TEXTURE_*_SAMPLINGMODE) */
enum pt_sampling { PT_SAMPLING_NEAREST = 1, PT_SAMPLING_BILINEAR = 2, PT_SAMPLING_TRILINEAR = 3 };

/* ---- context: replaces `new BABYLON.Engine(canvas, true)` (js/GLTF_Model_Path_Tracing.js:189).
 * A context has one or more parts, each one HIP stream on one gfx950 device. With several parts
 * every draw fans out inside pt_render: part k shades the 16-row bands b % N == k, screenOutput
 * pulls the +-2 halo rows from the band neighbours and part 0 gathers the RGBA8 bands into the
 * canvas (device-to-device copies over xGMI, ordered by HIP events). Render targets
 * stay distributed by bands; pt_read_pixels assembles them. Results are bit-identical to one part.
 * pt_ctx_create(device): one part on `device`. */
pt_ctx* pt_ctx_create(int device, int* err);
/* one part per set bit of device_mask (bit d = HIP device d), in increasing device order */
pt_ctx* pt_ctx_create_mask(uint32_t device_mask, int* err);
/* part k on devices[k]; a device may appear more than once (several parts on one GPU: the same
 * split, halo and gather path on a one-GPU host) */
pt_ctx* pt_ctx_create_devices(const int* devices, int n, int* err);
int pt_ctx_parts(const pt_ctx* ctx);
/* 1 when the halo pulls and the canvas gather between the context's distinct devices run as strided 2D
 * copies over peer access (xGMI), 0 when some pair has no peer access (hipDeviceCanAccessPeer false or
 * hipDeviceEnablePeerAccess failing; PT_PEER=0 forces it): they then run band by band through
 * hipMemcpyPeerAsync, same results. One-device contexts report 1. */
int pt_ctx_peer_copies(const pt_ctx* ctx);
void pt_ctx_destroy(pt_ctx* ctx);
const char* pt_last_error(pt_ctx* ctx);
int pt_sync(pt_ctx* ctx);
/* the default framebuffer ("canvas", RGBA8) that pt_render(effect, NULL) draws into;
 * replaces engine.resize()/getRenderWidth() (js/GLTF_Model_Path_Tracing.js:521-537) */
int pt_canvas_resize(pt_ctx* ctx, int width, int height);

/* ---- effects: replaces `new BABYLON.EffectWrapper({engine, fragmentShader, uniformNames,
 * samplerNames, name})` (js/GLTF_Model_Path_Tracing.js:773-811). The program is recognised from
 * the GLSL text; unknown text -> NULL with *err = PT_ERR_SHADER. Uniform/sampler names not in the
 * lists are ignored by the setters, as Babylon ignores undeclared uniforms. */
pt_effect* pt_effect_create(pt_ctx* ctx, const char* fragment_source,
                            const char* const* uniform_names, int n_uniforms,
                            const char* const* sampler_names, int n_samplers, int* err);
/* Same, with the program named directly (hosts that do not carry the reference's GLSL text,
 * e.g. the Python binding replaying a recorded uniform stream on the GPU box). */
pt_effect* pt_effect_create_program(pt_ctx* ctx, int program,
                                    const char* const* uniform_names, int n_uniforms,
                                    const char* const* sampler_names, int n_samplers, int* err);
void pt_effect_destroy(pt_effect* fx);
int pt_effect_program(const pt_effect* fx);

/* ---- uniforms: replaces effect.setFloat / setFloat2 / setFloat3 / setVector3 / setMatrix /
 * setInt / setBool (js/GLTF_Model_Path_Tracing.js:826-847). n = component count (1,2,3,4,16).
 * setBool is setInt(0|1), as in Babylon. Returns PT_OK also for ignored (undeclared) names. */
int pt_set_float(pt_effect* fx, const char* name, const float* v, int n);
int pt_set_int(pt_effect* fx, const char* name, int v);
/* effect.setTexture(sampler, texture) (js/GLTF_Model_Path_Tracing.js:818-825); tex NULL binds
 * nothing (an unloaded Babylon texture) */
int pt_set_texture(pt_effect* fx, const char* sampler, pt_texture* tex);

/* ---- textures -------------------------------------------------------------------------------
 * BABYLON.RawTexture.CreateRGBATexture(data, w, h, scene, mips, invertY, sampling, FLOAT)
 * (js/GLTF_Model_Path_Tracing.js:466-487): RGBA32F, data copied. */
pt_texture* pt_texture_create_rgba32f(pt_ctx* ctx, int width, int height, const float* data,
                                      int sampling, int invert_y, int* err);
/* new BABYLON.Texture(url, scene, noMipmap, invertY, sampling) of 8-bit images, decoded by the
 * host (js/GLTF_Model_Path_Tracing.js:749-758): RGBA8, data copied. */
pt_texture* pt_texture_create_rgba8(pt_ctx* ctx, int width, int height, const uint8_t* data,
                                    int sampling, int invert_y, int* err);
/* new BABYLON.RenderTargetTexture(name, {width,height}, scene, false, false, TEXTURETYPE_FLOAT,
 * false, NEAREST, ...) (js/GLTF_Model_Path_Tracing.js:762-768): RGBA32F, zero-filled. */
pt_texture* pt_render_target_create(pt_ctx* ctx, int width, int height, int* err);
/* MI355X extension: an RGBA32F render target over caller-owned device memory (w*h*16 bytes on
 * this context's device, e.g. a torch tensor that RCCL collectives also use). Not freed by
 * pt_texture_destroy; not resizable. */
pt_texture* pt_render_target_wrap(pt_ctx* ctx, int width, int height, void* device_ptr, int* err);
/* renderTarget.resize({width,height}) (js/GLTF_Model_Path_Tracing.js:529-530) */
int pt_render_target_resize(pt_texture* tex, int width, int height);
/* renderTarget.getSize() (js/GLTF_Model_Path_Tracing.js:826) */
int pt_texture_size(const pt_texture* tex, int* width, int* height);
void pt_texture_destroy(pt_texture* tex);

/* ---- draw: replaces eRenderer.render(effectWrapper, renderTargetOrNull)
 * (js/GLTF_Model_Path_Tracing.js:1230-1235). target NULL = the canvas. */
int pt_render(pt_effect* fx, pt_texture* target);
/* (A screenCopy draw may be deferred until the next draw: when that draw is the screenOutput of
 * the same source it writes the copy in the same pass. Every pt_* call that could observe the copy
 * target - another draw, read/write pixels, resize, destroy, pt_sync, pt_set_stream - runs it
 * first; code reading a wrapped render target's memory directly calls pt_sync before.) */

/* readPixels of a render target (RGBA32F, 16 B/texel) or of the canvas (tex NULL, RGBA8),
 * rows bottom-up; synchronises. */
int pt_read_pixels(pt_ctx* ctx, const pt_texture* tex, void* dst, size_t bytes);
/* MI355X extension (no reference counterpart: the page's canvas is the browser's). The canvas, as
 * pt_read_pixels(ctx, NULL, ...) would return it now, encoded on the device as a baseline sequential JFIF file:
 * 8-bit, three components, 4:4:4, the Annex K quantisation tables scaled by `quality` (1..100) and Huffman
 * tables, one restart interval per row of 8x8 MCUs; scanline 0 is canvas row height - 1 and alpha is ignored.
 * The bytes are those libjpeg-turbo writes for the same pixels and quality with 4:4:4 sampling and a restart
 * marker per MCU row (stage by stage: INTEGRATION.md "Encoding the canvas", tests/jpeg_enc_ref.py).
 * An observer like pt_read_pixels: a deferred screenCopy runs first, a context of several parts waits for the
 * gather and encodes part 0's gathered canvas, a row or output partition encodes the canvas as it stands; it
 * synchronises, and writes no texture, not the canvas, and no counter, statistic or timing window. Every stage
 * runs on the context's stream in context-owned workspace; the host copies the stream's length and then that
 * many bytes. *size receives the file's length. PT_ERR_ARG: capacity below that length (*size is then the
 * length needed and nothing is written to dst), quality outside 1..100, NULL dst or size, no canvas yet, a canvas
 * wider or taller than 65535 (the frame header's fields). */
int pt_canvas_encode_jpeg(pt_ctx* ctx, int quality, uint8_t* dst, size_t capacity, size_t* size);
/* The same with chroma subsampling; pt_canvas_encode_jpeg(ctx, q, ...) is pt_canvas_encode_jpeg_sub(ctx, q,
 * PT_JPEG_444, ...), and everything said there holds. Y is sampled hs x vs against Cb and Cr: 1x1 (4:4:4), 2x1
 * (4:2:2) or 2x2 (4:2:0); the bytes are those libjpeg-turbo writes for the same pixels and quality with that
 * subsampling and a restart marker per MCU row (tests/jpeg_enc_sub_ref.py). What the sampling changes:
 *   header   SOF0's Y sampling byte is hs << 4 | vs; DRI holds the MCUs of a row, ceil(W / (8 hs)).
 *   MCU      8 hs x 8 vs pixels; its blocks in coded order are the vs rows of hs Y blocks, then Cb, then Cr. One
 *            restart interval per MCU row; each component's DC prediction runs over its blocks in coded order and
 *            restarts at 0 with every MCU row.
 *   Y        the sample of pixel (min(x, W-1), min(y, H-1)).
 *   Cb, Cr   converted per full-resolution pixel (jccolor's fixed point), then downsampled as integers: the sample
 *            at column cx, row cy reads the columns min(2cx, W-1) and min(2cx+1, W-1) of, with cy' = min(cy,
 *            ceil(H / vs) - 1), the rows 2cy' and min(2cy'+1, H-1) (4:2:0) or the row cy' (4:2:2), and is
 *            (a + b + c + d + 1 + (cx & 1)) >> 2 (4:2:0) or (a + b + (cx & 1)) >> 1 (4:2:2).
 *   dummies  a Y block of an MCU outside the image's ceil(W / 8) x ceil(H / 8) blocks (W mod 16 in 1..8; for 4:2:0
 *            also H mod 16 in 1..8) is not computed from pixels: 63 zero ACs and the quantised DC of the block
 *            before it in the MCU, coded like any other block.
 * The transform, quantiser, Huffman tables, bit order, padding, stuffing and markers are those of 4:4:4.
 * PT_ERR_ARG also for a subsampling outside 0..2. */
enum pt_jpeg_subsampling { PT_JPEG_444 = 0, PT_JPEG_422 = 1, PT_JPEG_420 = 2 };   /* Pillow's numbering */
int pt_canvas_encode_jpeg_sub(pt_ctx* ctx, int quality, int subsampling,
                              uint8_t* dst, size_t capacity, size_t* size);
/* The same with the choice of Huffman tables; pt_canvas_encode_jpeg_sub(ctx, q, s, ...) is
 * pt_canvas_encode_jpeg_opt(ctx, q, s, 0, ...), and everything said there holds: it observes like pt_read_pixels and
 * synchronises, encodes part 0's gathered canvas on a context of several parts, writes no texture, counter,
 * statistic or timing window, and returns PT_ERR_ARG with *size set and dst untouched when capacity is too small.
 * optimize 0: the Annex K tables; the bytes, kernels and workspace of pt_canvas_encode_jpeg_sub.
 * optimize 1: Huffman tables built on the device for this canvas. The bytes are those libjpeg-turbo writes for the
 * same pixels, quality and subsampling with optimize_coding and a restart marker per MCU row
 * (tests/jpeg_enc_opt_ref.py); a decoder reconstructs the same pixels as from the optimize 0 file, which was 2 to
 * 30 % longer on rendered frames. What it changes:
 *   statistics  four histograms, DC 0, AC 0, DC 1, AC 1 (Y tables 0, Cb and Cr tables 1), of exactly the symbols
 *               coded: every block's DC category, per non-zero AC run >> 4 ZRLs and (run & 15) << 4 | size, an EOB
 *               when the last coefficient is zero; dummy Y blocks count.
 *   tables      libjpeg's jpeg_gen_optimal_table per histogram: a reserved symbol of count 1, Huffman's merges with
 *               the least count first and the largest symbol on a tie, code lengths limited to 16 in libjpeg's order,
 *               the reserved all-ones code removed, the symbols listed by length and then value.
 *   header      the same segments in the same order; each DHT carries its table's bits[16] and symbols, so the
 *               header's length (629 with the Annex K tables) varies with the pixels.
 * PT_ERR_ARG also for an optimize other than 0 or 1. */
int pt_canvas_encode_jpeg_opt(pt_ctx* ctx, int quality, int subsampling, int optimize,
                              uint8_t* dst, size_t capacity, size_t* size);
/* MI355X extension: the canvas, as pt_read_pixels(ctx, NULL, ...) would return it now, encoded on the device as a
 * PNG file, lossless: non-interlaced, 8 bits per sample, scanline 0 is canvas row height - 1. A browser's default
 * canvas serialisation (toBlob() / toDataURL() without a type) is a PNG. The definition is tests/png_enc_ref.py
 * (numpy and Python's zlib); stage by stage: INTEGRATION.md "Encoding the canvas: PNG".
 *   colour    PT_PNG_RGB writes colour type 2 and ignores alpha; PT_PNG_RGBA writes colour type 6, alpha as it
 *             stands. bpp is 3 or 4.
 *   filter    0..4: that PNG filter type on every row (None, Sub, Up, Average, Paeth). PT_PNG_ADAPTIVE: per row the
 *             type whose filtered row has the least sum of |byte as int8|, the lowest type on a tie. The filters are
 *             the PNG specification's: the row above the first is zeros, Average is floor((a + b) / 2) on unsigned
 *             values, Paeth prefers a when pa <= pb && pa <= pc, then b when pb <= pc.
 *   stream    height x (1 + bpp width) bytes, row by row: the filter byte, then the filtered bytes.
 *   deflate   the stream is cut into chunks of 16,320 bytes (the last one shorter, never empty). Chunk i is what zlib
 *             1.2.11 writes for compressobj(6, DEFLATED, 15, 8, Z_RLE) when it is fed that chunk in one compress()
 *             call followed by flush(Z_FULL_FLUSH), or flush(Z_FINISH) after the last: one block per chunk (stored,
 *             fixed or dynamic by zlib's size rule, with zlib's trees), tokens are literals and matches of distance 1
 *             within runs of equal bytes, runs do not cross chunks; every chunk starts on a byte boundary, a non-final
 *             one ends in the empty stored block 00 00 FF FF after padding; the two header bytes (78 01) precede the
 *             first chunk, the last has BFINAL set and is followed by the big-endian Adler-32 of the whole stream.
 *   file      the signature, IHDR, one IDAT per deflate chunk (so no CRC spans chunks), IEND.
 * It observes like pt_canvas_encode_jpeg: a deferred copy or blend runs first, a context of several parts encodes
 * part 0's gathered canvas, the call synchronises, and it writes no texture, not the canvas, and no counter,
 * statistic or timing window. All offsets are 64-bit and no canvas size is refused. *size receives the file's
 * length. PT_ERR_ARG: colour or filter out of range, NULL dst or size, no canvas yet, capacity below the file's
 * length (*size is then the length needed and dst is untouched).
 * The job form is pt_canvas_encode_png_begin, below. Out of scope: LZ77 matches beyond distance 1, 16-bit samples,
 * palettes, interlace, ancillary chunks. */
enum pt_png_colour { PT_PNG_RGB = 0, PT_PNG_RGBA = 1 };
enum pt_png_filter { PT_PNG_NONE = 0, PT_PNG_SUB = 1, PT_PNG_UP = 2, PT_PNG_AVERAGE = 3, PT_PNG_PAETH = 4,
                     PT_PNG_ADAPTIVE = 5 };
int pt_canvas_encode_png(pt_ctx* ctx, int colour, int filter, uint8_t* dst, size_t capacity, size_t* size);
/* MI355X extension: a render target's linear radiance, as pt_read_pixels(ctx, tex, ...) would return it now, encoded
 * on the device as a Radiance picture (.hdr, 32-bit_rle_rgbe): at most 4 B per texel and a sliver against the 16 of
 * the readback, and what pt_assets.decode_hdr and the JS shim decode. tex is an RGBA32F render target of the context
 * (a wrapped one too); alpha is ignored; scanline 0 is the target's row height - 1. The definition is
 * tests/hdr_enc_ref.py (numpy); every comparison with it is bytes ==.
 *   texel     every step one binary32 operation or exact. v = tex.xyz * scale; c_k = v_k > 0 ? min(v_k, cap) : +0 with
 *             cap = 255 x 2^119, the largest value RGBE holds (NaN, negatives and -0 give +0, +inf gives cap);
 *             m = max(max(c.x, c.y), c.z). m < 1e-32f: the texel is 0 0 0 0. Otherwise e = ((bits(m) >> 23) & 255) - 126,
 *             byte k is (int)floor(c_k x 2^(8 - e)), the fourth byte is e + 128: Radiance's setcolr with the factor
 *             256 / 2^e taken exactly. A decoder returns byte x 2^(E - 136), never above c_k and within m x 2^-7 of it.
 *   header    "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y H +X W\n", H and W in decimal.
 *   scanline  W < 8 or W > 32767: flat, the W texels as R G B E. Otherwise 02 02 W>>8 W&255, then the row's R, G, B
 *             and E planes, each coded on its own.
 *   plane     cut into maximal runs of equal bytes. A run of L bytes yields L / 127 run pieces of 127, then the
 *             remainder r = L % 127 as a run piece when r >= 4 and as r loose bytes otherwise. A run piece of n bytes
 *             of value b is 128 + n, b. Consecutive loose bytes form a stretch: one of 2 or 3 equal bytes is
 *             128 + n, b; any other is cut from its left into literals n, b_1 .. b_n of at most 128 bytes. This is the
 *             parse of Radiance's own scanline writer (MINRUN 4, counts below 128).
 *   bound     a coded plane is at most W + ceil(W / 128) bytes, so the file header + H (4 + 4 (W + ceil(W / 128))),
 *             or header + 4 W H for flat widths.
 * It observes like pt_read_pixels: a deferred screenCopy or a waiting blend that could change tex runs first, the call
 * synchronises, and it writes no texture, counter, statistic or timing window. Every stage runs on the context's
 * stream in context-owned workspace; all offsets are 64-bit. *size receives the file's length. PT_ERR_ARG before any
 * device work: a NULL ctx, a texture that is NULL, of another context or not a render target, a scale that is not
 * finite and > 0, NULL dst or size; PT_ERR_ARG also for a capacity below the file's length (*size is then the length
 * needed and dst is untouched). PT_ERR_UNSUPPORTED on a context of several parts, as pt_denoise.
 * Out of scope: XYZE, an EXPOSURE= header line, per-pixel weight normalisation (the caller's scale is the page's
 * uOneOverSampleCounter), contexts of several parts, byte equality with Radiance's own programs (the reference file
 * is the definition). Negatives, alpha, ids and named channels are pt_targets_encode_exr's, below. */
int pt_target_encode_hdr(pt_ctx* ctx, const pt_texture* tex, float scale,
                         uint8_t* dst, size_t capacity, size_t* size);
/* MI355X extension: render targets as one multi-channel OpenEXR file (single-part, scanlines, version 2, short
 * names), encoded on the device: the beauty accumulation with its feature buffers for a denoiser or a compositor, a
 * converged render archived without loss, signed normals and object ids that RGBE cannot hold. Channel i stores
 * component ch[i].component of ch[i].tex times ch[i].scale under ch[i].name as HALF or FLOAT; several channels may
 * name one texture; all textures have one size, RGBA32F render targets of the context (wrapped ones too). The
 * definition is tests/exr_enc_ref.py (numpy and zlib); every comparison with it is bytes ==. Little-endian throughout.
 *   head      76 2F 31 01, 02 00 00 00, then the attributes channels (chlist), compression, dataWindow and
 *             displayWindow (0, 0, W - 1, H - 1), lineOrder (0), pixelAspectRatio (1), screenWindowCenter (0, 0),
 *             screenWindowWidth (1), each as name\0 type\0 int32 size, value, then 00. A chlist entry is name\0,
 *             int32 type, 4 zero bytes (pLinear and reserved), int32 1, int32 1; the list ends with 00. Channels are
 *             stored sorted by name as unsigned bytes, whatever order ch has. 277 bytes for one channel "R", and
 *             len(name) + 17 for every other one.
 *   table     one uint64 per chunk: its offset in the file, in increasing y.
 *   chunk     int32 y of its first scanline, int32 data size, the data. It covers 1 scanline (PT_EXR_NONE,
 *             PT_EXR_ZIPS) or 16 (PT_EXR_ZIP), the last one what is left. Scanline y is the targets' row H - 1 - y. The
 *             block's raw bytes r are, per scanline, per channel in stored order, that channel's W samples.
 *   sample    v = x * scale, one binary32 multiply with denormals kept; a scale of exactly 1 takes x's bits as they
 *             are. FLOAT stores v's bits (0x7FC00000 for a NaN when scale is not 1). HALF rounds v to binary16, to
 *             nearest even, in integer arithmetic: subnormal halves are produced, what rounds past 65504 is +-inf,
 *             +-0 is kept, every NaN is 0x7E00.
 *   ZIPS/ZIP  with n the block's bytes and h = n / 2: t[i] = r[2 i], t[h + i] = r[2 i + 1]; p[0] = t[0],
 *             p[i] = t[i] - t[i - 1] + 128 mod 256. p is deflated as a zlib stream of its own the way
 *             pt_canvas_encode_png deflates its filtered stream: 78 01, a deflate block (zlib 1.2.11's bytes under
 *             Z_RLE, level 6) per 16,320-byte piece with a full flush behind each but the last, the Adler-32 of p. A
 *             stream shorter than n is the chunk's data; otherwise the data is r itself (OpenEXR's rule: a reader
 *             tells by size == n).
 *   bound     the head, 8 bytes of table and 8 of chunk head per chunk, and W H times the channels' sample bytes.
 * The contract is pt_target_encode_hdr's: it observes like pt_read_pixels (a deferred screenCopy or a waiting blend
 * that could change a named texture runs first), synchronises, writes no texture, counter, statistic or timing window,
 * runs on the context's stream in context-owned workspace with 64-bit offsets, and under a row partition encodes the
 * targets as they stand. *size receives the file's length. PT_ERR_ARG before any device work: n outside
 * 1..PT_EXR_CHANNELS_MAX, a texture that is NULL, of another context or not a render target, sizes that differ, a
 * component outside 0..3, a type or compression not listed, a scale that is not finite, a name that is NULL, empty,
 * longer than 31 bytes or holds a byte outside 0x21..0x7E, two equal names, NULL dst or size; PT_ERR_ARG also for a
 * capacity below the file's length (*size is then the length needed and dst is untouched). PT_ERR_UNSUPPORTED on a
 * context of several parts. PT_ERR_HIP (invalid value) for a block of 2^31 bytes or more, or more than 2^31 - 1 pieces.
 * Out of scope: tiles, multi-part and deep files, RLE / PIZ / PXR24 / B44 / DWA, UINT and subsampled channels, long
 * names, LZ77 matches beyond distance 1, per-pixel weight division (the accumulation's weight is uniform over a
 * frame, so the caller's scale is 1 / weight), contexts of several parts. No OpenEXR reader has read these files:
 * the layout is restated from OpenEXR's file-layout document and checked by the reference's own decoder. */
enum pt_exr_type { PT_EXR_HALF = 1, PT_EXR_FLOAT = 2 };                       /* OpenEXR's pixel-type numbers */
enum pt_exr_compression { PT_EXR_NONE = 0, PT_EXR_ZIPS = 2, PT_EXR_ZIP = 3 }; /* OpenEXR's numbers */
#define PT_EXR_CHANNELS_MAX 16
typedef struct pt_exr_channel {
    const char* name;        /* 1..31 bytes, each 0x21..0x7E, e.g. "R", "normal.X", "albedo.R", "id" */
    const pt_texture* tex;   /* an RGBA32F render target of ctx (wrapped ones too) */
    int component;           /* 0..3 */
    float scale;             /* finite */
    int type;                /* pt_exr_type */
} pt_exr_channel;
int pt_targets_encode_exr(pt_ctx* ctx, const pt_exr_channel* ch, int n, int compression,
                          uint8_t* dst, size_t capacity, size_t* size);
/* Encode and read jobs: pt_canvas_encode_jpeg_opt and pt_read_pixels(ctx, NULL, ...) without a host wait, for a
 * loop that serves every frame and keeps its frames in flight. begin enqueues the whole job on the context's stream
 * - the encoder's kernels into a device buffer of the job's own that holds the longest stream the canvas can have,
 * pt_jpeg_ship (or, for a read job, one copy) into pinned host memory, one event - and returns; the host goes on
 * queueing frames; finish waits for that job's event only, not for the stream.
 *   bytes    exactly what the synchronous call would have returned at the moment of begin: the same file for the
 *            same quality, subsampling and optimize, or the same width * height * 4 texels, rows bottom-up. Draws,
 *            pt_canvas_wrap switches and writes to a wrapped canvas queued later on the same stream do not change
 *            them. A wrapped canvas must stay alive until the jobs begun on it are done (poll says so, or finish
 *            or cancel returned).
 *   begin    makes no blocking HIP call once the buffers for the canvas's size exist; the first job at a size, after
 *            the canvas grew, or in a slot whose pinned buffer is smaller than the last files, allocates and so may
 *            wait. Unlike the synchronous calls it does NOT run a deferred screenCopy or a waiting blend
 *            (pt_fuse_stats does not move): the canvas is written by output passes only, each enqueued when its draw
 *            call returns, so it is complete in stream order. PT_ERR_ARG with *job NULL for what the synchronous call
 *            refuses (quality, subsampling, optimize, no canvas yet, a canvas wider or taller than 65535) and for a
 *            NULL job; PT_ERR_STATE when PT_JOBS_MAX jobs are pending (nothing is queued); PT_ERR_UNSUPPORTED on a
 *            context of several parts, whose canvas part 0 gathers under events of its own (the synchronous calls
 *            serve it).
 *   poll     hipEventQuery of the job's event; never blocks. *done 1 once finish would not wait.
 *   finish   waits for the job, copies into dst, sets *size and releases the job. Capacity too small: PT_ERR_ARG,
 *            *size is the length needed, dst is untouched and the job stays valid (call again). The pinned buffer
 *            is sized from the longest file so far and a quarter; of a file longer than that finish fetches the
 *            rest from the job's device buffer with a blocking copy of its own and the next jobs get more room
 *            (pt_job_stats out[2] counts these). NULL, a job already finished or cancelled: PT_ERR_ARG.
 *   cancel   releases a job without its bytes; waits for its device work, so a slot is never reused under a
 *            running kernel.
 * Jobs finish in any order. A handle is one of the context's PT_JOBS_MAX slots: it is dead once finish or cancel
 * returned PT_OK (a later begin may hand the same pointer out again) and with its context; pt_ctx_destroy waits for
 * pending jobs and frees them, and pt_canvas_resize waits before it frees the old canvas. A job writes no texture,
 * not the canvas, and no counter, statistic or timing window other than pt_job_stats: out[0] jobs begun, [1]
 * finished, [2] of those, finished through the slow copy, [3] cancelled.
 * pt_canvas_encode_png_begin and pt_target_encode_hdr_begin are the job forms of pt_canvas_encode_png and
 * pt_target_encode_hdr under the same contract: the synchronous call's bytes at the moment of begin, PT_ERR_ARG with
 * *job NULL for whatever that call refuses, PT_ERR_STATE with PT_JOBS_MAX pending, PT_ERR_UNSUPPORTED on a context of
 * several parts; poll, finish, cancel, the pinned buffer's growth and pt_job_stats as above. A slot's device buffer
 * holds the largest bound among the kinds of job it has served (JPEG stream, PNG IDATs, HDR scanlines); growing it may
 * wait, like any first job at a size. The PNG job, like the JPEG one, runs nothing deferred. The HDR job must make
 * tex what pt_read_pixels would return, so it enqueues a deferred screenCopy or a waiting blend first - it never
 * waits for it - and pt_fuse_stats may therefore move. A render target read by a pending job must outlive it:
 * pt_render_target_resize and pt_texture_destroy wait for the jobs on that texture, as pt_canvas_resize does for the
 * canvas; a wrapped target's memory is the caller's to keep alive likewise.
 * pt_targets_encode_exr_begin is pt_targets_encode_exr's job form under the HDR job's contract: it enqueues what is
 * deferred first and never waits for it, resize and destroy of any texture it names wait for it, the slot's device
 * buffer grows to the EXR bound, and the file's head is written at begin, so ch and its names need not outlive the
 * call. */
typedef struct pt_job pt_job;
#define PT_JOBS_MAX 4
int pt_canvas_encode_jpeg_begin(pt_ctx* ctx, int quality, int subsampling, int optimize, pt_job** job);
int pt_canvas_encode_png_begin(pt_ctx* ctx, int colour, int filter, pt_job** job);
int pt_target_encode_hdr_begin(pt_ctx* ctx, const pt_texture* tex, float scale, pt_job** job);
int pt_targets_encode_exr_begin(pt_ctx* ctx, const pt_exr_channel* ch, int n, int compression, pt_job** job);
int pt_canvas_read_begin(pt_ctx* ctx, pt_job** job);              /* the RGBA8 canvas, rows bottom-up */
int pt_job_poll(pt_job* job, int* done);                          /* never blocks */
int pt_job_finish(pt_job* job, uint8_t* dst, size_t capacity, size_t* size);
int pt_job_cancel(pt_job* job);
int pt_job_stats(pt_ctx* ctx, uint64_t out[4]);  /* begun, finished, finished through the slow copy, cancelled */
/* Upload rows of a render target (RGBA32F), used to seed the history buffer in tests and to
 * land gathered bands on the root in multi-GPU runs. */
int pt_write_pixels(pt_ctx* ctx, pt_texture* tex, const void* src, size_t bytes);

/* ---- MI355X extensions (no reference counterpart) -------------------------------------------
 * Row-band sharding for one-part contexts driven by one process per GPU (bench.py, torch.distributed;
 * a multi-part context shards itself and refuses these four: PT_ERR_ARG; pt_canvas_wrap then wraps
 * the gathered canvas): this context's path-tracing and screenCopy passes
 * shade only the 16-row bands b with b % num_parts == part (bands are whole 2x2 quads, so
 * derivatives are unchanged). num_parts = 1 restores full frames. */
int pt_set_row_partition(pt_ctx* ctx, int num_parts, int part);
/* screenOutput under the row partition too (enable = 1): only the owned bands of the output are
 * written. Its 5x5 filter reads the accumulation 2 rows beyond each band, so those halo rows must
 * hold the neighbouring ranks' values (babylon_pt.exchange_halos) before the draw. Default 0:
 * screenOutput shades the whole frame. */
int pt_set_output_partition(pt_ctx* ctx, int enable);
/* The canvas over caller-owned device memory: width*height RGBA8 texels, rows bottom-up (e.g. a
 * torch tensor that RCCL gathers from). Not freed by the context; pt_canvas_resize replaces it
 * with context-owned memory again. Re-wrapping another caller buffer is a host-side switch (no
 * synchronisation), so a caller can alternate between two canvases frame by frame. */
int pt_canvas_wrap(pt_ctx* ctx, int width, int height, void* device_ptr);
/* Path-tracing backend of this context: PT_BACKEND_MEGAKERNEL (default: one kernel, one lane per
 * path), PT_BACKEND_WAVEFRONT (per-segment kernels over compacted path queues) or
 * PT_BACKEND_PERSISTENT (waves regenerate finished lanes with new pixels; G-buffer + finish pass).
 * Results are bit-identical; the choice only changes speed. */
enum pt_backend { PT_BACKEND_MEGAKERNEL = 0, PT_BACKEND_WAVEFRONT = 1, PT_BACKEND_PERSISTENT = 2 };
int pt_set_backend(pt_ctx* ctx, int backend);
/* BVH walk of the glTF program. PT_BVH_PAIRS (default) re-packs tAABBTexture once per upload into
 * 64-byte child-pair records (both children's boxes in one line, pops without a fetch) and walks
 * those with the reference's short stack (LDS levels, deeper ones in a global slab); PT_BVH_TRAIL
 * walks the same records stacklessly: a restart trail of one bit per tree level plus a per-lane LDS
 * ring of the deepest pending entries, re-descending from a jump table of the top levels when the
 * ring runs dry (no stack memory beyond LDS; trees deeper than 28 levels - the reference's
 * stackLevels[28] - or whose nodes have more than one parent, keep PT_BVH_PAIRS). A texture whose
 * links are not exact in-range integers keeps PT_BVH_REFERENCE, the walk over the reference's own
 * texel pairs. Same nodes, same order, same results every way
 * (js/GLTFModelPathTracing_FragmentShader.js:211-298). Other values: PT_ERR_ARG.
 * pt_bvh_layout_used reports what the last glTF draw of the context walked (-1: none yet).
 * API change (round 4): the two-level layout PT_BVH_QUADS (3) was removed - it was slower on every
 * workload; pt_set_bvh_layout(ctx, 3) now returns PT_ERR_ARG and the Python
 * set_bvh_layout("quads") raises KeyError. */
enum pt_bvh_layout { PT_BVH_REFERENCE = 0, PT_BVH_PAIRS = 1, PT_BVH_TRAIL = 2 };
int pt_set_bvh_layout(pt_ctx* ctx, int layout);
int pt_bvh_layout_used(pt_ctx* ctx);
/* Enqueue this context's work on a caller-owned HIP stream (e.g. torch.cuda.current_stream(), so
 * that draws and RCCL collectives are ordered without host syncs); NULL restores the context's own
 * stream. The caller keeps the stream alive while the context uses it. */
int pt_set_stream(pt_ctx* ctx, void* hip_stream);
/* Device pointer of a render target's RGBA32F storage (for RCCL collectives from the host). From this call on the
 * texture counts as caller-visible, as wrapped memory does: everything deferred runs now, and the texels are current
 * on the context's stream after every draw. */
void* pt_texture_device_ptr(pt_texture* tex);
/* Device time of the last pt_render of each program kind, in ms (HIP events on the context
 * stream; requires pt_sync first). Draws are bracketed by events only once this has been called
 * (or with PT_DRAW_EVENTS=1): an event record costs ~5 us of stream time between kernels, so the
 * first call turns them on and returns PT_ERR_ARG; the draws after it are reported. */
int pt_last_render_ms(pt_ctx* ctx, int program, float* ms);
/* Timing window: between pt_timing_begin and pt_timing_end every draw is bracketed by its own
 * HIP event pair (no host sync inside the window); pt_timing_end closes the window, synchronises
 * and returns the summed device time and launch count of one program kind (further pt_timing_end
 * calls report other kinds from the same window). PT_TIMING_EVERY=k (read at pt_timing_begin)
 * brackets only every k-th draw of each program kind, so the events barely disturb the timed
 * stream; the launch count returned is then the bracketed draws'. */
int pt_timing_begin(pt_ctx* ctx);
int pt_timing_end(pt_ctx* ctx, int program, double* total_ms, int* launches);
/* Frame latency from the same timing window (closes it and synchronises, like pt_timing_end): for each
 * bracketed path-tracing draw of `program`, the device time from its begin event (recorded on the stream
 * its path tracing runs on, after the waits that order it: the moment its frame's path tracing may start)
 * to the end event of the next bracketed screenOutput draw (its canvas complete, main stream). Writes up
 * to `cap` values in window order and their count; with several parts, the slowest part's per frame. The
 * reference displays every frame it draws (js/GLTF_Model_Path_Tracing.js:1228-1237): with frames in
 * flight this is the draw-to-display delay the overlap adds. */
int pt_timing_latency(pt_ctx* ctx, int program, float* ms, int cap, int* n);
/* Algorithmic-byte counters: when enabled, path-tracing passes also accumulate
 * {paths, segments, node_fetches, leaf_tests, hit_lookups, rgba8_taps, stack_overflow, hdr_taps}. */
#define PT_NUM_COUNTERS 8
int pt_set_counting(pt_ctx* ctx, int enable);
int pt_read_counters(pt_ctx* ctx, uint64_t out[PT_NUM_COUNTERS]);
int pt_reset_counters(pt_ctx* ctx);
/* Wavefront queue statistics of the last path-tracing draw (synchronises): out[b] = paths entering
 * bounce b (b = 0..6), out[8 + b] = rays handed to the BVH walk at bounce b (b = 0..5); megakernel:
 * out[7] = the slowest tiles the next draw of the same target and program shades as 16-lane waves;
 * out[14] = late-bounce compaction of the last megakernel draw (PT_CONT: 0 off, 1 on, 2 auto = default):
 * bits 0-7: 0 off, 1 auto decided off, 2 auto decided on, 3 forced on, 4 auto trial running, 5 / 6 auto
 * before the trial, default on / off; bits 8-15: the frames that draw kept in flight (PT_OVERLAP_DEPTH, or 2
 * when the auto trial found two faster without compaction); bits 16-31: the path-tracing draws that
 * launched the late-bounce continuation (pt_cont) since the context was created, mod 2^16;
 * out[15] = the auto trial's time with
 * compaction per time without (at the faster depth), x 1000 (0 before the decision). */
int pt_queue_stats(pt_ctx* ctx, uint32_t out[16]);
/* Late-bounce compaction totals since the context was created (synchronises): out[0] = the path records
 * the path-tracing draws stored for the continuation kernel (pt_cont), out[1] = the draws that launched
 * it (not mod 2^16 as in pt_queue_stats); with several parts, summed over them. Each draw's history
 * blend adds its record count to the total as it zeroes it, so the path-tracing kernels pay nothing. */
int pt_cont_stats(pt_ctx* ctx, uint64_t out[2]);
/* The render loop's fused pass since the context was created (no device work, no synchronisation): out[0] = the
 * screenOutput draws that took the path-tracing draw's history blend and the frame's screenCopy along as one pass
 * (PT_FUSE_BLEND), out[1] = the screenCopy kernels launched on their own, for a copy target that
 * something had to see up to date; with several parts, summed over them (their frames never fuse: out[0] = 0). */
int pt_fuse_stats(pt_ctx* ctx, uint64_t out[2]);
/* Feature buffers: bind (or with NULLs unbind) feature targets to a path-tracing effect. Both are RGBA32F
 * render targets of the draw target's size; either may be NULL (that buffer is then not produced), both NULL
 * turns the feature off. While targets are bound, every pt_render of the effect also folds this draw's
 * G-buffer sample - CalculateRadiance's objectNormal / objectColor / objectID, the values the 2x2 edge test
 * reads - into them in place, on the owned 16-row bands, by the beauty's own history rule
 * (js/PathTracingCommon.js:1326-1337). With F = uFrameCounter, M = uCameraIsMoving,
 *   h = F == 1 ? 0 : (M ? 0.5 : 1)     (at F == 1 the history term is +0.0, still added)
 *   s = (F != 1 && M) ? 0.5 : 1
 *   normal_id.xyz     = h * old.xyz + s * objectNormal     normal_id.w     = objectID of this draw
 *   albedo_weight.xyz = h * old.xyz + s * objectColor      albedo_weight.w = h * old.w + s
 * so xyz / albedo_weight.w is the mean over the samples the beauty currently holds. The beauty target, the
 * canvas and every counter are bit for bit what they are without features. The fold runs on the context's
 * stream after the draw's own accumulation: a sync or a read comes after the folds of all earlier draws.
 * PT_ERR_ARG for a screenCopy / screenOutput effect or a texture that is not a render target of this
 * context; pt_render returns PT_ERR_STATE when a bound target's size differs from the draw target's, or
 * when it is the draw target, the bound previousBuffer or the other feature target. Destroying a bound
 * texture unbinds it. */
int pt_set_feature_targets(pt_effect* fx, pt_texture* normal_id, pt_texture* albedo_weight);
/* Denoising: the edge-avoiding a-trous filter (5x5 B3-spline taps at spacing 2^i in pass i, `iterations` of 1..5
 * passes) of a beauty target, guided by the feature buffers pt_set_feature_targets accumulated beside it. All four
 * textures are RGBA32F render targets of `ctx` (wrapped ones included) of one size; dst differs from the inputs.
 * Per pixel: w = albedo_weight.w, valid = w > 0, n = normal_id.xyz / w, id = normal_id.w, a = albedo_weight.xyz / w,
 * c = beauty.xyz / w, and d = demodulate ? c / max(a, 1e-3) : c. Each pass replaces d of a valid pixel by the
 * mean of the valid taps of its own id inside the image, weighted K[|dx|] K[|dy|] exp(-(|n_p - n_q|^2 /
 * sigma_normal^2 + |d_p - d_q|^2 / sigma_c^2)) with K = {3/8, 1/4, 1/16} and sigma_c = sigma_colour / 2^i. Then
 * dst = (d * max(a, 1e-3) if demodulated, else d) * w, dst.w = 1; an invalid pixel is (0, 0, 0, 1). So dst is in
 * the accumulation's scale with every sharpness flag saying "do not blur": screenOutput with dst bound as
 * accumulationBuffer is a plain tone map of it. Operation by operation: INTEGRATION.md "Denoising". A tap that
 * is skipped contributes nothing whatever it holds; a NaN in a valid pixel spreads over its footprint.
 * Asynchronous: enqueued on the context's stream after everything queued so far (a deferred screenCopy runs
 * first, as for any observer), before any later read or pt_sync; it does not synchronise, writes none of its
 * three inputs and changes no counter, statistic or timing window. Under pt_set_row_partition it filters the whole
 * frame, as screenOutput does by default: the caller supplies complete inputs.
 * PT_ERR_ARG, before any device work: a bad handle, a texture of another context or not a render target, sizes
 * that differ, dst equal to an input, iterations outside 1..5, a sigma that is not finite and > 0, demodulate
 * other than 0 or 1. PT_ERR_UNSUPPORTED: a context of several parts - its targets are distributed by 16-row
 * bands and the filter's footprint reaches +-32 rows; filtering across parts is out of scope. */
int pt_denoise(pt_ctx* ctx, const pt_texture* beauty, const pt_texture* normal_id,
               const pt_texture* albedo_weight, pt_texture* dst,
               int iterations, float sigma_normal, float sigma_colour, int demodulate);
/* Luminance moments: a third, independent feature target of a path-tracing effect (NULL unbinds it). `moments`
 * is an RGBA32F render target of the draw target's size. While it is bound, every pt_render of the effect also
 * folds the luminance of this draw's radiance r - CalculateRadiance's result, before the history rule and before
 * the x 0.5 of a moving camera - into it in place, on the owned 16-row bands, with h and s as for
 * pt_set_feature_targets above:
 *   L = (0.2126 * r.x + 0.7152 * r.y) + 0.0722 * r.z
 *   moments.x = h * old.x + s * L          moments.z = +0.0
 *   moments.y = h * old.y + s * (L * L)    moments.w = h * old.w + s
 * one IEEE binary32 operation per product and sum. So x / w and y / w are the first and second moment of the
 * luminance over the samples the beauty holds, and y / w - (x / w)^2 its variance. The fold is the feature
 * targets' (one launch, on the context's stream after the draw's own accumulation); with only this target bound a
 * draw stages no G-buffer. The beauty, the canvas, every counter, pt_queue_stats and pt_cont_stats are bit for
 * bit what they are without it. PT_ERR_ARG for a screenCopy / screenOutput effect or a texture that is not a
 * render target of this context; pt_render returns PT_ERR_STATE when its size differs from the draw target's, or
 * when it is the draw target, the bound previousBuffer or another bound feature target. Destroying the bound
 * texture unbinds it. */
int pt_set_moment_target(pt_effect* fx, pt_texture* moments);
/* Variance-guided denoising: pt_denoise's a-trous filter with its colour edge-stop replaced by a luminance one
 * that scales with each pixel's own variance (as in SVGF), so it blurs widely at 1 sample and lets go as the
 * image converges. The five textures are RGBA32F render targets of `ctx` of one size; dst differs from the
 * inputs. w, n, id, a, c, den = max(a, 1e-3) and d are pt_denoise's; mw = moments.w; lum(v) = (0.2126 v.x +
 * 0.7152 v.y) + 0.0722 v.z. A pixel is valid when w > 0 and mw > 0; an invalid pixel writes (0, 0, 0, 1) and is
 * skipped as a tap, like one outside the image or of another id.
 * Variance: vt = moments.y / mw - (moments.x / mw)^2, and vs the same from the sums of moments.x, .y, .w over the
 * kept taps of the 7x7 window; each 0 unless > 0. var = (mw < 4 ? vs : vt) / mw, the variance of the pixel's
 * mean, divided by lum(den)^2 when demodulating.
 * Pass i (spacing 2^i): gv = the mean of var over the kept taps of the 3x3 window at spacing 1 weighted {1/2, 1/4}
 * per axis; each kept tap q of the 5x5 B3 kernel weighs K K exp(-(|n_p - n_q|^2 / sigma_normal^2 + (lum(d_p) -
 * lum(d_q))^2 / (sigma_luminance^2 gv + 1e-8))); d' = sum wt d_q / sum wt, var' = sum wt^2 var_q / (sum wt)^2.
 * sigma_luminance is not halved between passes. The output is pt_denoise's: remodulated, times w, dst.w = 1.
 * Operation by operation: INTEGRATION.md "Denoising" and tests/denoise_var_ref.py.
 * The contract is pt_denoise's: asynchronous on the context's stream, writes only dst, changes no statistic or
 * timing window, filters the whole frame under a row partition. PT_ERR_ARG, before any device work: a bad handle,
 * a texture of another context or not a render target, sizes that differ, dst equal to an input, iterations
 * outside 1..5, a sigma that is not finite and > 0, demodulate other than 0 or 1. PT_ERR_UNSUPPORTED: a context of
 * several parts. */
int pt_denoise_variance(pt_ctx* ctx, const pt_texture* beauty, const pt_texture* normal_id,
                        const pt_texture* albedo_weight, const pt_texture* moments, pt_texture* dst,
                        int iterations, float sigma_normal, float sigma_luminance, int demodulate);
/* Ray queries: SceneIntersect of a path-tracing effect's program on caller-given rays. For each of `n` world-space
 * rays (origins[3i..3i+2], dirs[3i..3i+2]) hits[i] holds exactly what the effect's program computes in
 * SceneIntersect for that ray: the uniforms and data textures are the ones bound now (SetupScene, the model
 * matrix, the material switches, the BVH and triangle textures), the walk is the one pt_set_bvh_layout selects, the
 * query is the closest hit, and nothing of CalculateRadiance is computed. It needs no render target, previousBuffer
 * or blue noise, and no draw before it. The direction is taken as given: t is in units of its length (for a
 * normalised direction t is a distance, and a valid uFocusDistance for a camera ray). A component that is zero,
 * negative zero, infinite or NaN is an input like any other: the record is what the arithmetic gives. On a miss
 * t is the shaders' INFINITY constant (1000000.0), object_id -1, type -100, triangle -1 and every other field +0.0.
 * Synchronous: the call is queued on the context's stream after everything queued so far (so a pt_write_pixels
 * into a BVH texture before it is seen) and returns with `hits` filled. It observes no render target, so a deferred
 * screenCopy stays deferred; it writes no texture, counter, statistic, cost table, tile order or timing window, and
 * the walk's stack levels beyond LDS go to a slab of the call's own, never the draws': a draw after it gives the bits
 * it gives without it, with several frames in flight too. Rays and records pass through context-owned device
 * staging that grows on demand; a large call runs in chunks inside the one call. A mesh deeper than the shaders'
 * stackLevels[28] is reported as for a draw: by the next pt_sync, as PT_ERR_DATA.
 * PT_ERR_ARG, before any device work: a bad handle, a screenCopy / screenOutput effect, n < 0, a NULL pointer with
 * n > 0. n == 0 is PT_OK and touches nothing. PT_ERR_UNSUPPORTED: a context of several parts, as pt_denoise.
 * PT_ERR_STATE: a mesh program without tAABBTexture / tTriangleTexture bound as RGBA32F data textures. */
typedef struct pt_ray_hit {          /* 64 bytes, one line per ray */
    float   t;                       /* SceneIntersect's hitT; INFINITY (1000000.0) on a miss */
    int32_t object_id;               /* hitObjectID; -1 on a miss */
    int32_t type;                    /* hitType (the shaders' material constants); -100 on a miss */
    int32_t triangle;                /* mesh hit: the triangle's index in tTriangleTexture (8 texels each); else -1 */
    float   normal[3];               /* hitNormal, world space, as SceneIntersect leaves it (not normalised again; the
                                        bump map applied where the program applies it) */
    float   bary_u;                  /* mesh hit: the walk's triU; else 0 */
    float   color[3];                /* hitColor as SceneIntersect writes it (1,1,1 for the mesh) */
    float   bary_v;                  /* mesh hit: the walk's triV; else 0 */
    float   uv[2];                   /* mesh hit: the interpolated hit uv; else 0 */
    float   reserved[2];             /* +0.0 */
} pt_ray_hit;
int pt_cast_rays(pt_effect* fx, const float* origins, const float* dirs, int n, pt_ray_hit* hits);
/* Ray queries with a distance bound, an occlusion mode and device-resident rays. pt_cast_rays is the
 * PT_RAYS_HOST + PT_RAYS_CLOSEST + t_max == NULL case of it, and stays as it is to the bit.
 * The bound. With t_max given, ray i is SceneIntersect with hitT starting at min(INFINITY, t_max[i]) instead of
 * INFINITY - the GLSL's min, y < x ? y : x - and nothing else changed. So a NaN, an infinite or any t_max >= 1000000.0
 * is no bound; and since every object test is `d < hitT`, strict, a t_max of 0, of -1, or of exactly the unbounded
 * hit's t is a miss. A ray that takes no object gets pt_cast_rays' miss record: t = 1000000.0 (not t_max), ids
 * -1 / -100 / -1, the rest +0. t is in units of |dir|: with dirs = q - p and t_max = 1 the query is the open segment
 * from p to q.
 * The bound is the walk's, not a filter on the unbounded record. For the analytic objects the two are the same (a
 * running minimum under a strict `<`). For the mesh they are not: the lower hitT also culls boxes, so a triangle whose
 * t is below the bound is not found when the slab test of its leaf (or of a node above it) gives a distance that is
 * not - which happens within an ulp or so of the bound, on all three BVH layouts alike, and is what the GLSL with
 * that start would do. A surface that close to the segment's end may or may not count, as in any ray tracer: a host
 * that aims at a surface point shortens the segment.
 * PT_RAYS_OCCLUDED: out[i] = 1 iff the bounded closest-hit record of ray i has object_id >= 0, else 0; which object
 * is not said. The walk may stop at the first occluder; the flag does not depend on whether it does, nor on the
 * BVH layout.
 * PT_RAYS_HOST: pt_cast_rays' contract - host pointers, context-owned staging, chunks, synchronous - with 4 B more
 * per ray going in when t_max is given; OCCLUDED copies back 1 B per ray.
 * PT_RAYS_DEVICE: origins, dirs, t_max and out are memory of the context's device (a torch tensor's data_ptr(),
 * say). The call enqueues on the context's stream (pt_set_stream applies) after everything queued so far and returns
 * without synchronising; there is no staging copy - the kernel reads the caller's rays and writes the caller's
 * output, one launch per 262,144 rays at pointer offsets, with a context-owned slab for the walk's deep stack levels
 * only. The caller keeps all buffers alive and untouched until it has synchronised (pt_sync, or its own stream), and
 * orders what produced the rays before the call (the context's stream, or an earlier synchronise). out for CLOSEST
 * must be 16-byte aligned (the records are written as 16-byte stores); origins, dirs and t_max 4-byte aligned.
 * Everything pt_cast_rays promises holds for both: no render target observed; no counter, statistic, cost table, tile
 * order or timing window moved; the draws' slabs never touched; a draw after it gives the bits it gives without it.
 * Errors as pt_cast_rays, before any device work; also PT_ERR_ARG for a NULL q, an unknown mode or memory, or a
 * misaligned device pointer. n == 0 is PT_OK and touches nothing. PT_ERR_UNSUPPORTED: a context of several parts. */
enum { PT_RAYS_CLOSEST = 0, PT_RAYS_OCCLUDED = 1 };     /* pt_ray_query::mode */
enum { PT_RAYS_HOST = 0, PT_RAYS_DEVICE = 1 };          /* pt_ray_query::memory: where every pointer of the query lives */
typedef struct pt_ray_query {
    const float* origins;            /* [3n] */
    const float* dirs;               /* [3n] */
    const float* t_max;              /* [n], or NULL: no bound */
    void*        out;                /* CLOSEST: pt_ray_hit[n]; OCCLUDED: uint8_t[n], each 1 or 0 */
    int          n, mode, memory;
} pt_ray_query;
int pt_cast_rays_ex(pt_effect* fx, const pt_ray_query* q);
/* Device self-test of the pinned GLSL built-ins (ops as the oracle's pto_math_probe). */
int pt_math_probe(pt_ctx* ctx, int op, const float* x, const float* y, float* out, int n);
/* Exhaustive device self-test of a fast built-in sequence against the IEEE operation it replaces,
 * over all 2^32 binary32 inputs: op 0 = the reciprocal (grcp vs 1.0f/x), op 1 = the square root
 * (gsqrt vs sqrtf). Writes the mismatch count. */
int pt_math_exhaustive(pt_ctx* ctx, int op, uint64_t* mismatches);
/* BVH_Build_Iterative(workList, aabb_array) (js/BVH_Fast_Builder.js:320-406) as native host code:
 * aabb_in = the per-triangle AABBs the setup script fills (9 floats: min.xyz, max.xyz,
 * centroid.xyz; js/GLTF_Model_Path_Tracing.js:421-454), work = the triangle ids to build over
 * (n of them). Writes 8 floats per node, depth-first, exactly the reference's tAABBTexture layout
 * and bits, and returns the node count (2n-1), or a negative pt_status (max_nodes too small). No
 * context or device needed. */
int pt_bvh_build(const float* aabb_in, const uint32_t* work, int n, float* nodes_out, int max_nodes);
/* The same build on a gfx950 device (csrc/pt_bvh_gpu.hip): level by level, every node of a depth
 * split together, the same tree and bits as pt_bvh_build (js/BVH_Fast_Builder.js:43-406; the page
 * runs it at js/GLTF_Model_Path_Tracing.js:456-462). aabb_in holds 9 floats for every triangle id
 * up to the largest in work; n <= 2^24. Synchronous. Returns the node count (2n-1) or a negative
 * pt_status; *ms_out (may be NULL) = device time of the build, uploads and read-back excluded. */
int pt_bvh_build_gpu(int device, const float* aabb_in, const uint32_t* work, int n, float* nodes_out,
                     int max_nodes, float* ms_out);
/* JPEG decode for the hosts' texture loading: replaces the browser's decode of the glTF models'
 * map images, which the glTF loader hands to `new BABYLON.Texture` (js/GLTF_Model_Path_Tracing.js:
 * 252-274) and the page binds with effect.setTexture (:822-825). libjpeg-turbo's default
 * decompression reproduced bit for bit (csrc/pt_jpeg.cpp: baseline and progressive, accurate
 * integer IDCT, fancy upsampling, RGB output); RGBA8 rows top first, alpha 255. pt_jpeg_size reads
 * the frame header; pt_jpeg_decode_rgba8 needs capacity >= 4 * width * height. Host code: no
 * context or device. PT_ERR_UNSUPPORTED for arithmetic-coded, 12-bit, CMYK or stored-RGB files. */
int pt_jpeg_size(const uint8_t* data, size_t size, int* width, int* height);
int pt_jpeg_decode_rgba8(const uint8_t* data, size_t size, uint8_t* rgba, size_t capacity);
/* Library identity: "libpt <version> gfx950" */
const char* pt_version(void);

#ifdef __cplusplus
}
#endif
#endif
