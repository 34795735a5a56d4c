"""The definition of pt_target_encode_hdr's file (include/pt.h), in numpy: a render target's RGBA32F texels, rows
bottom-up, as a Radiance picture (32-bit_rle_rgbe). Every comparison with it is bytes ==.

Two forms of the plane coder: `code_plane`, the rules as pt.h states them (maximal runs, run pieces of 127, a
remainder of 4 or more as a piece and of less as loose bytes, stretches of loose bytes as a short token or as literals
of 128 at most), and `code_plane_sequential`, the loop of Radiance's own scanline writer (MINRUN 4, counts below
128), byte by byte from the left. tests/test_hdr_enc_ref.py holds them equal.

`certificate` says what a case reaches in the kernels' geometry (csrc/pt_hdr_enc.hip: a wave per plane, steps of
STEP bytes and then of STEP runs, WAVES waves at most; a lane per texel, TEXELS a trip), so a test can assert that it still reaches what it is for."""
import numpy as np

MINRUN, MAXRUN, MAXLIT = 4, 127, 128
STEP, WAVES = 64, 2048          # pth::kStep, pth::kWaves
TEXELS = 4096 * 256             # pth::kPlaneGrid blocks of 256 lanes: the texels one trip of pt_hdr_planes converts
CAP = np.uint32(0x7EFF0000).view(np.float32)   # 255 x 2^119
TINY = np.float32(1e-32)


def flat_width(w):
    return w < 8 or w > 32767


def header(w, h):
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)


def plane_max(w):
    return w + (w + 127) // 128


def file_max(w, h):
    return len(header(w, h)) + (4 * w * h if flat_width(w) else h * (4 + 4 * plane_max(w)))


def rgbe(rgb, scale):
    """(..., 3) float32 -> (..., 4) uint8; every step one binary32 operation or exact"""
    rgb = np.asarray(rgb, np.float32)
    with np.errstate(all="ignore"):
        v = rgb * np.float32(scale)
        c = np.where(v > 0, np.minimum(v, CAP), np.float32(0)).astype(np.float32)
        m = c.max(axis=-1)
        dark = m < TINY
        e = ((m.view(np.uint32) >> 23) & 255).astype(np.int32) - 126
        e = np.where(dark, 0, e)
        f = ((8 - e + 127).astype(np.uint32) << 23).view(np.float32)   # 2^(8 - e), a normal number
        q = np.floor(c * f[..., None])
    out = np.empty(rgb.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.where(dark[..., None], 0, q).astype(np.uint8)
    out[..., 3] = np.where(dark, 0, e + 128).astype(np.uint8)
    return out


def decoded(rgbe8):
    """what the project's decoders return for RGBE bytes: byte x 2^(E - 136), 0 for E = 0 (float64, exact)"""
    e = rgbe8[..., 3].astype(np.int64)
    return np.where(e[..., None] > 0, np.ldexp(rgbe8[..., :3].astype(np.float64), (e - 136)[..., None]), 0.0)


def runs_of(plane):
    """the maximal runs of a byte plane: (starts, lengths)"""
    p = np.asarray(plane, np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(p[1:] != p[:-1]) + 1))
    return starts, np.diff(np.concatenate((starts, [len(p)])))


def tokens(plane):
    """the plane's tokens by the rules: a list of ("run" | "short" | "literal", position, count)"""
    p = np.asarray(plane, np.uint8)
    starts, lens = runs_of(p)
    out, loose = [], []   # loose: the positions of the open stretch

    def close():
        if not loose:
            return
        if 2 <= len(loose) <= 3 and len({int(p[i]) for i in loose}) == 1:
            out.append(("short", loose[0], len(loose)))
        else:
            for k in range(0, len(loose), MAXLIT):
                out.append(("literal", loose[k], len(loose[k:k + MAXLIT])))
        loose.clear()

    for s, L in zip(starts.tolist(), lens.tolist()):
        at = s
        for _ in range(L // MAXRUN):
            close()
            out.append(("run", at, MAXRUN))
            at += MAXRUN
        r = L % MAXRUN
        if r >= MINRUN:
            close()
            out.append(("run", at, r))
        else:
            loose.extend(range(at, at + r))   # (consecutive positions: a stretch is contiguous)
    close()
    return out


def code_plane(plane):
    p = np.asarray(plane, np.uint8)
    out = bytearray()
    for kind, at, n in tokens(p):
        if kind == "literal":
            out.append(n)
            out += p[at:at + n].tobytes()
        else:
            out.append(128 + n)
            out.append(int(p[at]))
    return bytes(out)


def code_plane_sequential(plane):
    """Radiance's scanline writer for one component, as a loop over the bytes"""
    p = bytes(np.asarray(plane, np.uint8).tobytes())
    n = len(p)
    out = bytearray()
    j = 0
    while j < n:
        beg, cnt = j, 0
        while beg < n:   # find the next run
            cnt = 1
            while cnt < MAXRUN and beg + cnt < n and p[beg + cnt] == p[beg]:
                cnt += 1
            if cnt >= MINRUN:
                break
            beg += cnt
        if 1 < beg - j < MINRUN and all(p[k] == p[j] for k in range(j + 1, beg)):   # a short run
            out.append(128 + beg - j)
            out.append(p[j])
            j = beg
        while j < beg:   # the non-run
            c2 = min(beg - j, MAXLIT)
            out.append(c2)
            out += p[j:j + c2]
            j += c2
        if cnt >= MINRUN and beg < n:   # the run
            out.append(128 + cnt)
            out.append(p[beg])
            j += cnt
    return bytes(out)


def scanlines(tex, scale):
    """(H, W, 4) float32 rows bottom-up -> (H, W, 4) uint8 RGBE, scanline 0 first"""
    tex = np.asarray(tex, np.float32)
    return rgbe(tex[::-1, :, :3], scale)


def encode(tex, scale=1.0):
    q = scanlines(tex, scale)
    h, w = q.shape[:2]
    out = bytearray(header(w, h))
    for y in range(h):
        if flat_width(w):
            out += q[y].tobytes()
        else:
            out += bytes((2, 2, w >> 8, w & 255))
            for k in range(4):
                out += code_plane(q[y, :, k])
    return bytes(out)


def certificate(tex, scale=1.0):
    """what the image reaches: the token kinds, the longest literal and run, the planes at their bound, and in the
    kernels' geometry: steps of bytes and of runs, a run across a byte step, a stretch across a run step, planes
    beyond the waves in flight, texels beyond one trip of the conversion's grid"""
    q = scanlines(tex, scale)
    h, w = q.shape[:2]
    cert = dict(flat=flat_width(w), kinds=set(), literal=0, run=0, at_bound=0, byte_steps=-(-w // STEP), run_steps=0,
                run_across_byte_step=False, stretch_across_run_step=False, plane_loop=4 * h > WAVES,
                texel_loop=w * h > TEXELS,
                literal_lengths=set(), run_lengths=set())
    if cert["flat"]:
        return cert
    for y in range(h):
        for k in range(4):
            p = q[y, :, k]
            starts, lens = runs_of(p)
            cert["run_steps"] = max(cert["run_steps"], -(-len(starts) // STEP))
            cert["run_lengths"].update(lens.tolist())
            if np.any(starts // STEP != (starts + lens - 1) // STEP):
                cert["run_across_byte_step"] = True
            # run j, j a multiple of STEP, goes on the stretch of the run before it: both are loose alone
            for j in range(STEP, len(starts), STEP):
                if lens[j] < MINRUN and lens[j - 1] % MAXRUN in (1, 2, 3):
                    cert["stretch_across_run_step"] = True
            size = 0
            for kind, _, n in tokens(p):
                cert["kinds"].add(kind)
                if kind == "literal":
                    cert["literal"] = max(cert["literal"], n)
                    cert["literal_lengths"].add(n)
                    size += n + 1
                else:
                    cert["run"] = max(cert["run"], n)
                    size += 2
            cert["at_bound"] += size == plane_max(w)
    return cert
