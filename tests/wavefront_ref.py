"""A plain float64 restatement of the path tracer's Generate, Shade and Connect stages (the contract of include/tinybvh_amd.h over
wavefront.cl:52-287 and tools.cl), vectorised in numpy, with a rounding-error bound for every float it returns.

How the bounds are derived.  Every float is a pair (value in float64, bound on |device float32 value - value|), class F.  The inputs are the
float32 records the device itself produced (exact, bound 0).  The kernels are built without contraction and without fast-math, so each +, -, *, /
and sqrtf of the kernel is one correctly rounded float32 operation: it adds U * |result| (U = 2^-24, half an ulp) to the bound its operands carry
into the result, and the operands' bounds go through the operation to first order (a product's by the other factor, a quotient's by 1 / divisor,
a root's by the exact difference of roots).  That is `k * 2^-23 * scale` applied operation by operation instead of once per field: every rounding
on a value's chain contributes half an ulp of the magnitude it happened at, so cancellation (a small sum of large terms) is covered by the terms'
magnitudes, not by the result's.  Operations that cannot round are not counted: a product with 0, +-1 or a power of two, a sum with 0, integer to
float conversions below 2^24, the RNG (WangHash, xorshift32, >> 8 times 2^-24: exact integers).  cosf / sinf add TRIG_ULP ulps of their result
(the OpenCL full-profile bound the device library is built to) plus their argument's bound.  Second-order terms are included where they are one
multiplication away (e_a * e_b); the rest is below 2^-24 of the bound.

Roundings per field (what a single factor k in k * 2^-23 * scale would have to count; the code below IS the count):
  Generate   D      jitter 2, point on the screen 5, minus eye 1, normalise 5 + 0.5 sqrt + 1 reciprocal + 1 product
  Shade      N      edges 2 x 1, cross 3, (instance: 5), normalise as above
             I      2 (t * D, + O)
             shadow O: I + L * eps 2 on top of I and L;  D = L: light point 2, minus I 1, length 5 + sqrt, reciprocal, product
                    tmax: length, minus 2 eps 1;  contribution: T * ipdf 1, colour 1 (+ 1 blue-noise / colour byte scale), light 1, g (MIS: solid angle 4,
                    reciprocal 1, sum 2, ratio 2; point light 3), product 1
             bounce D: mirror: dot 5, product 1, difference 1;  diffuse: Malley basis (cross 3 + normalise, cross 3), sqrt 2, trig 2 x (1 + TRIG_ULP),
                    products 2, combination 5, normalise;  pdf: dot 5, max, 1 / pi 1;  T: colour 1, k3 1 on top
  Accumulator       the bound of each contribution + (additions into the pixel) * U * (sum of |contribution|), for both images of a difference

Decisions at rounding level (`nd > 0`, `ndl > 0`, `ldist > 2 eps`, `solid > 0`, the min(2 pi, .) clamp, `|N.x| > 0.9`): the quantity and its bound are
returned; a path whose quantity lies within its bound of the threshold is UNDECIDED at that stage, and `flip` (one bit per decision) evaluates the
other side, so that a test can hold the device to the side it took.  `hit.t < 1e30` is exact."""
import numpy as np

U = 2.0 ** -24
TRIG_ULP = 4.0          # sinf / cosf: at most 4 ulp (OpenCL full profile)
FAR = float(np.float32(1e30))
PATH_LAST_SPECULAR, PATH_VIA_DIFFUSE = 1, 2
MATERIAL_LIGHT, MATERIAL_SPECULAR = 1, 2
f32 = lambda x: float(np.float32(x))
INV_PI, TWO_PI, FOUR_PI, BYTE = f32(0.31830988), f32(6.2831853), f32(12.566371), f32(0.00392)
# decisions, one flip bit each
DEC_ND, DEC_NDL, DEC_LDIST, DEC_SOLID, DEC_CLAMP, DEC_NX = 1, 2, 4, 8, 16, 32
DECISIONS = {"nd": DEC_ND, "ndl": DEC_NDL, "ldist": DEC_LDIST, "solid": DEC_SOLID, "clamp": DEC_CLAMP, "nx": DEC_NX}


class F:
    """A float32 quantity of the kernel: v = its value in float64, e = a bound on |what the device holds - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, F) else F(x)

    @staticmethod
    def _trivial(a):   # a factor that cannot make a product round: 0, +-1, +-2, +-0.5, exactly known
        return (a.e == 0) & ((a.v == 0) | (np.abs(a.v) == 1) | (np.abs(a.v) == 2) | (np.abs(a.v) == 0.5))

    def __add__(self, o):
        o = F.of(o)
        v = self.v + o.v
        exact = ((self.e == 0) & (self.v == 0)) | ((o.e == 0) & (o.v == 0))
        return F(v, self.e + o.e + np.where(exact, 0.0, U * np.abs(v)))

    __radd__ = __add__

    def __neg__(self):
        return F(-self.v, self.e)

    def __sub__(self, o):
        return self + (-F.of(o))

    def __rsub__(self, o):
        return F.of(o) + (-self)

    def __mul__(self, o):
        o = F.of(o)
        v = self.v * o.v
        exact = F._trivial(self) | F._trivial(o)
        return F(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + np.where(exact, 0.0, U * np.abs(v)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = F.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            den = np.maximum(np.abs(o.v) - o.e, 1e-300)
            return F(v, (self.e + np.abs(v) * o.e) / den + U * np.abs(v))

    def __rtruediv__(self, o):
        return F.of(o) / self


def fsqrt(a):
    v = np.sqrt(np.maximum(a.v, 0.0))
    lo = np.sqrt(np.maximum(a.v - a.e, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(a.e > 0, a.e / np.where(v + lo > 0, v + lo, 1.0), 0.0)
    e = np.where((a.e > 0) & (v + lo == 0), np.sqrt(a.e), e)
    return F(v, e + U * v)


def fabs(a):
    return F(np.abs(a.v), a.e)


def fmin(a, b):
    a, b = F.of(a), F.of(b)
    return F(np.minimum(a.v, b.v), np.maximum(a.e, b.e))


def fmax(a, b):
    a, b = F.of(a), F.of(b)
    return F(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def where(c, a, b):
    a, b = F.of(a), F.of(b)
    return F(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def ftrig(fn, a):
    v = fn(a.v)
    return F(v, a.e + TRIG_ULP * 2 * U * np.abs(v))


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def norm3(a):
    l = fsqrt(dot(a, a))
    r = where(l.v == 0, 0.0, 1.0 / where(l.v == 0, 1.0, l))
    return tuple(c * r for c in a)


def vec(a):
    """(n, 3) float32 -> three exact F."""
    a = np.asarray(a)
    return tuple(F(a[..., k].astype(np.float64)) for k in range(3))


def stack(v):
    return np.stack([c.v + np.zeros(np.broadcast(*[x.v for x in v]).shape) for c in v], -1), np.stack([np.broadcast_to(c.e, np.broadcast(*[x.v for x in v]).shape) for c in v], -1)


# ---- the integer RNG: exact ------------------------------------------------------------------------------------------------

def wang(s):
    s = np.asarray(s, np.uint32)
    with np.errstate(over="ignore"):
        s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16)); s = s * np.uint32(9); s = s ^ (s >> np.uint32(4)); s = s * np.uint32(0x27d4eb2d)
        return s ^ (s >> np.uint32(15))


def rnd_stream(s, count):
    """`count` draws of xorshift32 from state s (0 replaced by 1): floats (s >> 8) * 2^-24, exact."""
    s = np.where(s == 0, np.uint32(1), s).astype(np.uint32)
    out = []
    for _ in range(count):
        s = s ^ (s << np.uint32(13)); s = s ^ (s >> np.uint32(17)); s = s ^ (s << np.uint32(5))
        out.append((s >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
    return out


def generate_seed(seed, gindex):
    with np.errstate(over="ignore"):
        return wang(np.uint32(seed) * np.uint32(9781) + np.asarray(gindex, np.uint32) * np.uint32(6271) + np.uint32(1))


def shade_seed(seed, gpixel, depth):
    with np.errstate(over="ignore"):
        return wang(np.uint32(seed) * np.uint32(7919) + np.asarray(gpixel, np.uint32) * np.uint32(2699) + np.uint32(depth) * np.uint32(104729) + np.uint32(17))


def blue_noise_index(gpixel, height, page):
    """Noise() of wavefront.cl:24-31 as Shade calls it: x = pixel % height, y = pixel / height, a 128 x 128 page."""
    gpixel = np.asarray(gpixel, np.uint32)
    nx = (gpixel % np.uint32(height)) & np.uint32(127); ny = (gpixel // np.uint32(height)) & np.uint32(127)
    return (np.uint32(page) << np.uint32(14)) + (ny << np.uint32(7)) + nx


def path_word(pixel, depth, flags):
    return (np.asarray(pixel, np.uint32) << np.uint32(8)) | np.uint32((depth & 15) << 4) | np.asarray(flags, np.uint32)


def clamp_depth(max_depth):
    return 3 if max_depth == 0 else min(int(max_depth), 8)


# ---- Generate --------------------------------------------------------------------------------------------------------------

def generate(cam, seed, first_row=0, band_rows=None):
    """Camera rays of rows [first_row, first_row + band_rows) of the image cam describes, in queue order (4 x 4 tiles of the band): O exact, D with its
    bound, the path word."""
    W, Hf = int(cam.width), int(cam.height)
    H = Hf if band_rows is None else int(band_rows)
    n = W * H
    i = np.arange(n, dtype=np.uint32)
    in_tile = i & 15; tile = i >> 4; tiles_x = W // 4
    px = (tile % tiles_x) * 4 + (in_tile & 3); py = (tile // tiles_x) * 4 + (in_tile >> 2)
    r0, r1 = rnd_stream(generate_seed(seed, i + np.uint32(first_row * W)), 2)
    u = (F(px.astype(np.float64)) + F(r0)) / float(W)
    v = (F((py + first_row).astype(np.float64)) + F(r1)) / float(Hf)
    eye, p1, p2, p3 = (tuple(F(f32(x)) for x in a) for a in (cam.eye, cam.p1, cam.p2, cam.p3))
    P = tuple(p1[k] + u * (p2[k] - p1[k]) + v * (p3[k] - p1[k]) for k in range(3))
    D = norm3(tuple(P[k] - eye[k] for k in range(3)))
    return {"n": n, "O": np.array([f32(x) for x in cam.eye], np.float32), "D": D, "word": path_word(py * W + px, 0, PATH_LAST_SPECULAR), "pixel": py * W + px}


# ---- Shade -----------------------------------------------------------------------------------------------------------------

class Params:
    """tbvh_wf_params as the kernel sees them (every float through float32), plus what the wavefront object adds."""

    def __init__(self, light_pos, light_color=(1.0, 1.0, 1.0), sky_lo=(0.6, 0.7, 0.8), sky_hi=(0.2, 0.4, 0.9), eps=1e-3, max_depth=3, seed=1,
                 light_size=(0.0, 0.0), one_diffuse_bounce=False, reference_letter=False, sample_index=0xFFFFFFFF, blue_noise=None,
                 width=0, height=0, pixel_offset=0):
        g = lambda a: [f32(x) for x in a]
        self.light_pos, self.light_color, self.sky_lo, self.sky_hi, self.light_size = g(light_pos), g(light_color), g(sky_lo), g(sky_hi), g(light_size)
        self.eps, self.max_depth, self.seed = f32(eps), clamp_depth(max_depth), int(seed)
        self.one_diffuse_bounce, self.letter, self.sample_index = bool(one_diffuse_bounce), bool(reference_letter), int(sample_index) & 0xFFFFFFFF
        self.blue_noise = None if blue_noise is None else np.ascontiguousarray(blue_noise, np.uint32).reshape(-1)
        self.width, self.height, self.pixel_offset = int(width), int(height), int(pixel_offset)


class Geometry:
    """Where Shade finds a hit's triangle: one vertex array, or (TLAS) the instance records and one vertex array per BLAS."""

    def __init__(self, verts=None, instances=None, blas_verts=None):
        self.verts, self.instances, self.blas_verts = verts, instances, blas_verts

    def triangle(self, rays):
        prim = rays["prim"].astype(np.int64)
        if self.instances is None:
            tri = self.verts.reshape(-1, 3, 4)[prim]
            return tri, None
        inst = rays["inst"].astype(np.int64)            # byte 44 of the hit record
        blas = self.instances["blasIdx"][inst]
        tri = np.zeros((rays.shape[0], 3, 4), np.float32)
        for b, v in enumerate(self.blas_verts):
            m = blas == b
            tri[m] = v.reshape(-1, 3, 4)[prim[m]]
        return tri, self.instances["invTransform"][inst].reshape(-1, 4, 4)


def shade(rays, aux, geo, P, depth, flip=0):
    """One Shade stage over the live entries `rays` (RAY_DTYPE with Extend's hit records) and `aux` (PATH_AUX_DTYPE) of a path queue.  flip: an int or an
    array of DEC_* bits, the decisions to take the other way.  Returns a dict; every float field is a (value, bound) pair of (n, 3) / (n,) arrays."""
    n = rays.shape[0]
    flip = np.broadcast_to(np.asarray(flip, np.int64), (n,))
    dec = {}

    def decide(name, q, thr, relevant):
        q = F.of(q)
        qe = np.broadcast_to(q.e, q.v.shape)
        dec[name] = {"undecided": relevant & (np.abs(q.v - thr) <= qe), "relevant": relevant}
        return (q.v > thr) ^ ((flip & DECISIONS[name]) != 0)

    word = aux["pixel"]
    pixel = (word >> np.uint32(8)).astype(np.int64); pflags = (word & np.uint32(15)).astype(np.int64)
    T = vec(aux["T"])
    brdf_pdf = rays["instIdx"].view(np.float32).astype(np.float64)      # D.w of the record: the postponed pdf
    with np.errstate(divide="ignore"):
        ipdf = where(brdf_pdf > 0, F(1.0) / F(np.where(brdf_pdf > 0, brdf_pdf, 1.0)), 0.0)
    O, D = vec(rays["O"]), vec(rays["D"])
    t = F(rays["t"].astype(np.float64))
    area = P.light_size[0] > 0 and P.light_size[1] > 0
    light_area = F(P.light_size[0]) * F(P.light_size[1])
    miss = ~(rays["t"] < np.float32(1e30))
    hit_rays = rays.copy(); hit_rays["prim"][miss] = 0; hit_rays["inst"][miss] = 0
    tri, inv = geo.triangle(hit_rays)
    mat_word = tri[:, 0, 3].copy().view(np.uint32)
    mtype = (mat_word >> np.uint32(24)).astype(np.int64)
    emitter = ~miss & (mtype == MATERIAL_LIGHT)
    surface = ~miss & ~emitter
    specular = surface & (mtype == MATERIAL_SPECULAR)
    diffuse = surface & ~specular
    zero3 = tuple(F(np.zeros(n)) for _ in range(3))

    # sky (wavefront.cl:151-156; weighted by the postponed pdf unless to the letter)
    k = 0.5 * (D[1] + 1.0)
    ws = F(1.0) if P.letter else ipdf
    sky = tuple((T[c] * ws) * (F(P.sky_lo[c]) + k * (F(P.sky_hi[c]) - F(P.sky_lo[c]))) for c in range(3))
    # emitter (wavefront.cl:163-178)
    mis_light = emitter & ((pflags & PATH_LAST_SPECULAR) == 0) & area
    tt = where(mis_light, t, 1.0)
    x = light_area / (tt * tt) * fabs(D[1])
    solid = fmin(TWO_PI, x)          # (continuous in x, and the weight is continuous in solid at 0: no decision to flip on this branch)
    pos = solid.v > 0
    light_pdf = where(pos, 1.0 / where(pos, solid, 1.0), FAR)
    w_mis = F(0.0) if P.letter else 1.0 / (light_pdf + F(brdf_pdf))
    w = where(mis_light, w_mis, ipdf)
    emit = tuple((T[c] * w) * F(P.light_color[c]) for c in range(3))
    term = tuple(where(miss, sky[c], where(emitter, emit[c], 0.0)) for c in range(3))

    # surface
    T = tuple(T[c] * ipdf for c in range(3))
    v0, v1, v2 = vec(tri[:, 0, :3]), vec(tri[:, 1, :3]), vec(tri[:, 2, :3])
    e1 = tuple(v1[c] - v0[c] for c in range(3)); e2 = tuple(v2[c] - v0[c] for c in range(3))
    N = cross(e1, e2)
    if inv is not None:   # the transposed inverse takes the normal to world space
        M = [[F(inv[:, r, c].astype(np.float64)) for c in range(3)] for r in range(3)]
        N = tuple(M[0][c] * N[0] + M[1][c] * N[1] + M[2][c] * N[2] for c in range(3))
    N = norm3(N)
    nd = dot(N, D)
    flipN = decide("nd", nd, 0.0, surface)
    N = tuple(where(flipN, -N[c], N[c]) for c in range(3))
    ts = where(surface, t, 0.0)
    I = tuple(O[c] + ts * D[c] for c in range(3))
    rgb = (mat_word & np.uint32(0xffffff)).astype(np.int64)
    color = tuple(where(rgb != 0, F(((rgb >> s) & 255).astype(np.float64)) * BYTE, f32(0.7)) for s in (16, 8, 0))
    gpixel = (pixel + P.pixel_offset).astype(np.uint32)
    r0, r1, r2, r3 = (F(r) for r in rnd_stream(shade_seed(P.seed, gpixel, depth), 4))
    if P.blue_noise is not None and depth == 0 and P.sample_index < 4:
        w0 = P.blue_noise[blue_noise_index(gpixel, P.height, P.sample_index * 2)]; w1 = P.blue_noise[blue_noise_index(gpixel, P.height, P.sample_index * 2 + 1)]
        b = lambda x: F(x.astype(np.float64)) * BYTE
        r2, r3 = b(w0 >> np.uint32(16)), b((w0 >> np.uint32(8)) & np.uint32(255))      # noise0 -> the light sample
        r0, r1 = b(w1 >> np.uint32(16)), b((w1 >> np.uint32(8)) & np.uint32(255))      # noise1 -> the bounce
    # next event estimation (wavefront.cl:205-222)
    lp = [F(x) for x in P.light_pos]
    Pl = (lp[0] + (r2 - 0.5) * F(P.light_size[0]), lp[1], lp[2] + (r3 - 0.5) * F(P.light_size[1])) if area else tuple(lp)
    L = tuple(Pl[c] - I[c] for c in range(3))
    ldist = fsqrt(dot(L, L))
    lpos = ldist.v > 0
    il = where(lpos, 1.0 / where(lpos, ldist, 1.0), 0.0)
    L = tuple(L[c] * il for c in range(3))
    ndl = dot(N, L)
    two_eps = 2.0 * P.eps
    ok_ndl = decide("ndl", ndl, 0.0, diffuse)
    ok_dist = decide("ldist", ldist, two_eps, diffuse)
    want_shadow = diffuse & ok_ndl & ok_dist
    if area:
        xs = light_area * il * il * fabs(L[1])
        over = decide("clamp", xs, TWO_PI, want_shadow)
        solid_s = where(over, TWO_PI, xs)
        spos = decide("solid", solid_s, 0.0, want_shadow)
        lpdf = where(spos, 1.0 / where(solid_s.v != 0, solid_s, 1.0), FAR)
        g = (INV_PI * ndl) / (lpdf + ndl * INV_PI)
    else:
        g = ndl * il * il * INV_PI
    contrib = tuple(T[c] * color[c] * F(P.light_color[c]) * g for c in range(3))
    sh_O = tuple(I[c] + L[c] * P.eps for c in range(3))
    sh_tmax = ldist - two_eps

    # the bounce (wavefront.cl:225-242)
    more = depth + 1 < P.max_depth
    k2 = 2.0 * dot(N, D)
    R_spec = tuple(D[c] - k2 * N[c] for c in range(3))
    stopped = (pflags & PATH_VIA_DIFFUSE) != 0 if P.one_diffuse_bounce else np.zeros(n, bool)
    bounce_diffuse = diffuse & more & ~stopped
    if P.letter:   # tools.cl:34-39: a half sphere about the world z axis added to N
        rl = fsqrt(fmax(1.0 - r1 * r1, 0.0)); pl = FOUR_PI * r0
        R_diff = norm3((N[0] + ftrig(np.cos, pl) * rl, N[1] + ftrig(np.sin, pl) * rl, N[2] + r1))
    else:          # Malley: a cosine-weighted direction about N
        rr, cz, phi = fsqrt(r1), fsqrt(1.0 - r1), TWO_PI * r0
        big_x = decide("nx", fabs(N[0]), f32(0.9), bounce_diffuse)
        t1 = (where(big_x, 0.0, 1.0), where(big_x, 1.0, 0.0), F(np.zeros(n)))      # the tangent's seed: the y axis where N is near the x axis, else the x axis
        bx = norm3(cross(t1, N))
        by = cross(N, bx)
        cx, cy = ftrig(np.cos, phi) * rr, ftrig(np.sin, phi) * rr
        R_diff = norm3(tuple(cz * N[c] + cx * bx[c] + cy * by[c] for c in range(3)))
    ndr = fmax(dot(N, R_diff), f32(1e-6))
    pdf_d = ndr * INV_PI
    T_diff = tuple(T[c] * color[c] * pdf_d for c in range(3))
    T_spec = tuple(T[c] * color[c] for c in range(3))
    want_bounce = (specular & more) | bounce_diffuse
    R = tuple(where(specular, R_spec[c], R_diff[c]) for c in range(3))
    b_O = tuple(I[c] + R[c] * P.eps for c in range(3))
    b_T = tuple(where(specular, T_spec[c], T_diff[c]) for c in range(3))
    b_pdf = where(specular, 1.0, pdf_d)
    new_flags = np.where(specular, PATH_LAST_SPECULAR, PATH_VIA_DIFFUSE)
    if not area:
        dec["clamp"] = dec["solid"] = {"undecided": np.zeros(n, bool), "relevant": np.zeros(n, bool)}
    if P.letter:
        dec["nx"] = {"undecided": np.zeros(n, bool), "relevant": np.zeros(n, bool)}
    if area:   # the emitter branch's clamp and `solid > 0`: nothing to flip (see there), but a path at the threshold counts as undecided all the same
        xe = np.broadcast_to(x.e, x.v.shape)
        dec["clamp"]["undecided"] = dec["clamp"]["undecided"] | (mis_light & (np.abs(x.v - TWO_PI) <= xe))
        dec["solid"]["undecided"] = dec["solid"]["undecided"] | (mis_light & (np.abs(solid.v) <= xe))
    und_bits = np.zeros(n, np.int64)
    for name, d in dec.items():
        und_bits |= np.where(d["undecided"], DECISIONS[name], 0)
    return {
        "n": n, "pixel": pixel, "flags": pflags, "miss": miss, "emitter": emitter, "specular": specular, "diffuse": diffuse, "mis_light": mis_light,
        "term": stack(term), "terminal": miss | emitter,
        "want_shadow": want_shadow, "shadow_O": stack(sh_O), "shadow_D": stack(L), "shadow_tmax": (sh_tmax.v, np.broadcast_to(sh_tmax.e, sh_tmax.v.shape)),
        "contrib": stack(contrib),
        "want_bounce": want_bounce, "bounce_O": stack(b_O), "bounce_D": stack(R), "bounce_pdf": (b_pdf.v + np.zeros(n), np.broadcast_to(b_pdf.e, (n,))),
        "bounce_T": stack(b_T), "bounce_word": path_word(pixel, depth + 1, new_flags),
        "ndl_rejected": diffuse & ~ok_ndl, "stopped": diffuse & more & stopped,
        "undecided": und_bits, "decisions": dec,
    }


# ---- records out of the reference: the complete path tracer on the CPU (tests/test_wavefront_ref_host.py) --------------------

def safercp(x):
    x = np.asarray(x, np.float32)
    big = np.abs(x) > np.float32(1e-12)
    with np.errstate(divide="ignore"):
        return np.where(big, np.float32(1.0) / np.where(big, x, np.float32(1.0)), np.where(x >= 0, np.float32(1e30), np.float32(-1e30))).astype(np.float32)


def make_queue(ray_dtype, aux_dtype, O, D, dw, tmax, T, word):
    n = D.shape[0]
    r = np.zeros(n, ray_dtype); a = np.zeros(n, aux_dtype)
    r["O"] = np.broadcast_to(np.asarray(O, np.float32), (n, 3)); r["mask"] = 0xFFFF
    r["D"] = D.astype(np.float32); r["instIdx"] = np.broadcast_to(np.asarray(dw, np.float32), (n,)).copy().view(np.uint32)
    r["rD"] = safercp(r["D"]); r["t"] = np.broadcast_to(np.asarray(tmax, np.float32), (n,))
    a["T"] = np.broadcast_to(np.asarray(T, np.float32), (n, 3)); a["pixel"] = word
    return r, a
