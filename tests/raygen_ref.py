"""References for the device ray generators and the ray-bin key, written from the contract in include/tinybvh_amd.h ("wavefront
path-tracing helpers", tbvh_bin_rays_device) and the reference lines it cites — tiny_bvh_speedtest.cpp:526-549 (primary), :564-587
(bounce), :859-865 (shadow), tools.cl:9-11 (WangHash, xorshift32), tiny_bvh.h:442 (safercp), :506-510 (normalize), :695-703 (the Ray
constructor) — and NOT from the kernels.  Plain numpy; nothing here needs a GPU.

Each generator comes twice:

  *_f32   the documented operations, one numpy float32 operation per C operation, in C's evaluation order (a + b + c = (a + b) + c; no
          fused sums, no linalg.norm).  The library is built without contraction and with HIP's correctly rounded divide and square root,
          so the device should give these bits.
  *_f64   the same formulas in float64 on the float32 inputs, with everything integer (pixel mapping, hash, xorshift draws) exact and
          the draw itself — float32(draw) * float32(2.3283064365387e-10) — taken over unchanged.  It also returns, per component, a
          bound on how far a float32 evaluation may lie from it (see "The bound" below).

What the records are: the Ray constructor normalises the direction it is given and sets rD = safercp(D), mask = 0xFFFF, hit.t = tmax,
everything else 0.
  primary  Ray( eye, P - eye ), P = p1 + u (p2 - p1) + v (p3 - p1).  (The speedtest hands the constructor an already normalised
           P - eye, so it normalises twice; tinybvh_amd.rays.primary and the library normalise once.  The second pass moves D by an
           ulp at most, far inside the bound, and it is noted here so that nobody takes it for an oversight.)
  bounce   R = normalize( draws - 0.5 ); hit (t < 1e30): I = O + t D, N = normalize( cross( v1 - v0, v2 - v0 ) ), N reversed if
           dot( N, D ) > 0, R reversed if dot( N, R ) < 0; miss: I = O + 20 D; Ray( I + 0.001f R, R ).
  shadow   t = min( 1000, hit.t ), I = O + t D, Ld = normalize( light - I ), Ray( I + Ld eps, Ld, length( light - I ) - eps ).
A xorshift32 state of 0 never leaves 0; the header does not say what a generator does with it, so the references reject such input
(seeds_ok) instead of guessing.

The bound.  u = 2^-24.  A float32 +, -, *, / or sqrt returns the exact result of its operands times (1 + d), |d| <= u, so it adds
at most u |result| to whatever error its operands carry (standard running error analysis, first order in u):
  x = a op b (+, -)      e(x) <= e(a) + e(b) + u |x|
  x = a * b              e(x) <= |b| e(a) + |a| e(b) + u |x|
  normalize( v )         l = sqrt( (x x + y y) + z z ): three roundings under the root (relative 3 u, halved by it: 1.5 u), the root
                         1 u, rl = 1 / l 1 u, v rl 1 u: 4.5 u |D_c|, taken as NORM_OPS = 5 to cover the second-order terms; an input
                         error e(v) moves D by ( I - D D^T ) e(v) / |v|, a projection, so by at most |e(v)|_2 / |v| per component.
  length( v )            2.5 u |v| + |e(v)|_2, taken as 3 u |v| + |e(v)|_2.
Primary rays, for instance: p2 - p1 and p3 - p1 one rounding each, u and v one (the division; the integers convert exactly), the two
products, two sums and P - eye one each: with M the largest coordinate of the pyramid that is e(dir_c) <= 16 u M, so
|D - D64| <= u ( 5 + 16 sqrt(3) M / |dir| ) per component — 2^-23 ( 2.5 + 14 M / |dir| ), the size the operation count predicts; the code
below does not use M but the actual magnitudes, ray by ray, which is tighter."""
import numpy as np

from tinybvh_amd import RAY_DTYPE

F = np.float32
U = 2.0 ** -24
NORM_OPS = 5.0
FAR = F(1e30)
DRAW_SCALE = F(2.3283064365387e-10)
BOUNCE_OFFSET = F(0.001)
MISS_DISTANCE = F(20.0)
SHADOW_TMAX = F(1000.0)
KNIFE = 1e-6          # bounce: a sign decision may differ from float64 where |dot| is below this
KNIFE_CAP = 1e-3      # ... for at most this share of a batch


# ---- integers: pixel mapping, hash, draws ------------------------------------------------------------------------------------------------

def pixel_map(width, height, spp_x, spp_y, first, n):
    """(numerator of u, numerator of v) of rays first .. first + n - 1: sample i % spp of pixel i / spp, pixels in 4x4 tiles, tiles row by
    row, x fastest inside a tile; sample s sits at (s % spp_x, s / spp_x) of the pixel's spp_x x spp_y grid."""
    assert width > 0 and height > 0 and width % 4 == 0 and height % 4 == 0 and spp_x > 0 and spp_y > 0
    i = np.arange(n, dtype=np.uint64) + np.uint64(first)
    spp = np.uint64(spp_x * spp_y)
    s = i % spp
    pix = i // spp
    tile, in_tile = pix // np.uint64(16), pix % np.uint64(16)
    tiles_x = np.uint64(width // 4)
    px = (tile % tiles_x) * np.uint64(4) + in_tile % np.uint64(4)
    py = (tile // tiles_x) * np.uint64(4) + in_tile // np.uint64(4)
    return px * np.uint64(spp_x) + s % np.uint64(spp_x), py * np.uint64(spp_y) + s // np.uint64(spp_x)


def wang_hash(s):
    s = np.array(s, dtype=np.uint32, ndmin=1)
    with np.errstate(over="ignore"):
        s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16))
        s = s * np.uint32(9)
        s = s ^ (s >> np.uint32(4))
        s = s * np.uint32(0x27d4eb2d)
        return s ^ (s >> np.uint32(15))


def ray_seeds(seed, index):
    """WangHash( seed + i * 747796405 + (i >> 32) ), in 32-bit arithmetic, i = the 64-bit index of the ray within the call."""
    i = np.array(index, dtype=np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        lo = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(747796405)
        return wang_hash(np.uint32(seed & 0xFFFFFFFF) + lo + (i >> np.uint64(32)).astype(np.uint32))


def xorshift_draws(state, k=3):
    """k successive xorshift32 outputs (13, 17, 5) per state: (n, k) uint32."""
    s = np.array(state, dtype=np.uint32, ndmin=1)
    out = np.empty((s.shape[0], k), np.uint32)
    for j in range(k):
        s = s ^ (s << np.uint32(13))
        s = s ^ (s >> np.uint32(17))
        s = s ^ (s << np.uint32(5))
        out[:, j] = s
    return out


def seeds_ok(seed, n):
    return bool((ray_seeds(seed, np.arange(n, dtype=np.uint64)) != 0).all())


def bounce_draws(seed, n):
    """(n, 3) float32 in [0, 1]: float32( draw ) * float32( 2.3283064365387e-10 )."""
    st = ray_seeds(seed, np.arange(n, dtype=np.uint64))
    assert (st != 0).all(), "a zero xorshift state: not specified, choose another seed"
    return xorshift_draws(st).astype(F) * DRAW_SCALE


# ---- float32 building blocks -------------------------------------------------------------------------------------------------------------

def safercp_f32(x):
    """tinybvh_safercp: 1 / x if x > 1e-12 or x < -1e-12, else (x >= 0 ? 1e30 : -1e30); -0.0 >= 0, a NaN is not."""
    x = np.asarray(x, F)
    big = (x > F(1e-12)) | (x < F(-1e-12))
    return np.where(big, F(1) / np.where(big, x, F(1)), np.where(x >= 0, FAR, -FAR)).astype(F)


def _dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _length32(v):
    return np.sqrt(_dot32(v, v))


def _normalize32(v):
    l = _length32(v)
    rl = np.where(l == 0, F(0), F(1) / np.where(l == 0, F(1), l))
    return v * rl[:, None]


def _cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def records(O, direction, tmax):
    """Ray( O, direction, tmax ) per row, all in float32."""
    assert O.dtype == F and direction.dtype == F   # (a float64 array here would mean an operation above was not done in float32)
    r = np.zeros(O.shape[0], RAY_DTYPE)
    D = _normalize32(direction)
    assert D.dtype == F
    r["O"] = O
    r["D"] = D
    r["rD"] = safercp_f32(D)
    r["mask"] = 0xFFFF
    r["t"] = tmax
    return r


def _cam(cam):
    return [np.array(list(v), F) for v in (cam.eye, cam.p1, cam.p2, cam.p3)]


# ---- float64 building blocks: value and bound --------------------------------------------------------------------------------------------

def _norm2(e):
    return np.sqrt((e * e).sum(axis=1))


def _normalize64(v, ev):
    """normalize( v ) and the bound on a float32 normalize of a vector within ev of v."""
    l = _norm2(v)
    zero = l == 0
    ls = np.where(zero, 1.0, l)
    D = np.where(zero[:, None], 0.0, v / ls[:, None])
    prop = np.where(zero, np.where(_norm2(ev) == 0, 0.0, np.inf), _norm2(ev) / ls)
    return D, NORM_OPS * U * np.abs(D) + prop[:, None]


def _length64(v, ev):
    l = _norm2(v)
    return l, 3 * U * l + _norm2(ev)


def _tri_normal64(verts, prim):
    tri = np.asarray(verts, F).reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    v0, v1, v2 = tri[prim, 0], tri[prim, 1], tri[prim, 2]
    N = np.cross(v1 - v0, v2 - v0)
    l = _norm2(N)
    return np.where((l == 0)[:, None], 0.0, N / np.where(l == 0, 1.0, l)[:, None])


# ---- primary -----------------------------------------------------------------------------------------------------------------------------

def primary_f32(cam, first, n):
    eye, p1, p2, p3 = _cam(cam)
    nu, nv = pixel_map(cam.width, cam.height, cam.spp_x, cam.spp_y, first, n)
    u = nu.astype(F) / F(cam.width * cam.spp_x)
    v = nv.astype(F) / F(cam.height * cam.spp_y)
    a, b = p2 - p1, p3 - p1
    P = (p1[None, :] + u[:, None] * a[None, :]) + v[:, None] * b[None, :]
    return records(np.broadcast_to(eye, P.shape), P - eye[None, :], FAR)


def primary_f64(cam, first, n):
    eye, p1, p2, p3 = [x.astype(np.float64) for x in _cam(cam)]
    nu, nv = pixel_map(cam.width, cam.height, cam.spp_x, cam.spp_y, first, n)
    u = (nu.astype(np.float64) / float(cam.width * cam.spp_x))[:, None]
    v = (nv.astype(np.float64) / float(cam.height * cam.spp_y))[:, None]
    a, b = (p2 - p1)[None, :], (p3 - p1)[None, :]
    ua, vb = u * a, v * b                       # a and u carry one rounding each, the product a third
    s1 = p1[None, :] + ua; e1 = 3 * U * np.abs(ua) + U * np.abs(s1)
    P = s1 + vb; eP = e1 + 3 * U * np.abs(vb) + U * np.abs(P)
    d = P - eye[None, :]; ed = eP + U * np.abs(d)
    D, eD = _normalize64(d, ed)
    return {"O": np.broadcast_to(eye, D.shape).copy(), "eO": np.zeros_like(D), "D": D, "eD": eD,
            "t": np.full(n, float(FAR)), "et": np.zeros(n)}


# ---- bounce ------------------------------------------------------------------------------------------------------------------------------

def bounce_f32(rays, verts, seed):
    n = rays.shape[0]
    O, D, t = rays["O"], rays["D"], rays["t"]
    R = _normalize32(bounce_draws(seed, n) - F(0.5))
    hit = t < FAR
    tri = np.asarray(verts, F).reshape(-1, 3, 4)[:, :, :3]
    p = np.where(hit, rays["prim"], 0)
    N = _normalize32(_cross32(tri[p, 1] - tri[p, 0], tri[p, 2] - tri[p, 0]))
    N = np.where((_dot32(N, D) > 0)[:, None], -N, N)
    R = np.where((hit & (_dot32(N, R) < 0))[:, None], -R, R)
    tt = np.where(hit, t, MISS_DISTANCE)
    I = O + tt[:, None] * D
    return records(I + BOUNCE_OFFSET * R, R, FAR)


def bounce_f64(rays, verts, seed):
    """Besides O, D and their bounds: `knife` (the rays whose sign decisions float32 may take the other way) and O_alt, D_alt, eO_alt (what
    such a ray becomes with R reversed: either decision going the other way reverses R, nothing else)."""
    n = rays.shape[0]
    O, D, t = rays["O"].astype(np.float64), rays["D"].astype(np.float64), rays["t"]
    R0 = bounce_draws(seed, n).astype(np.float64) - 0.5
    R, eR = _normalize64(R0, U * np.abs(R0))
    hit = t < FAR
    N = _tri_normal64(verts, np.where(hit, rays["prim"], 0))
    nd = (N * D).sum(axis=1)
    N = np.where((nd > 0)[:, None], -N, N)
    nr = (N * R).sum(axis=1)
    knife = hit & ((np.abs(nd) < KNIFE) | (np.abs(nr) < KNIFE))
    R = np.where((hit & (nr < 0))[:, None], -R, R)
    tt = np.where(hit, t, MISS_DISTANCE).astype(np.float64)[:, None]
    tD = tt * D
    I = O + tD; eI = U * np.abs(tD) + U * np.abs(I)
    c = float(BOUNCE_OFFSET)
    out = {"knife": knife, "t": np.full(n, float(FAR)), "et": np.zeros(n)}
    for sign, suffix in ((1.0, ""), (-1.0, "_alt")):
        Oo = I + c * sign * R
        out["O" + suffix] = Oo
        out["eO" + suffix] = eI + c * eR + U * c * np.abs(R) + U * np.abs(Oo)
        out["D" + suffix], out["eD" + suffix] = _normalize64(sign * R, eR)
    return out


# ---- shadow ------------------------------------------------------------------------------------------------------------------------------

def shadow_f32(rays, light, eps):
    light = np.asarray(light, F); eps = F(eps)
    t = np.minimum(SHADOW_TMAX, rays["t"])
    I = rays["O"] + t[:, None] * rays["D"]
    L = light[None, :] - I
    Ld = _normalize32(L)
    return records(I + Ld * eps, Ld, _length32(L) - eps)


def shadow_f64(rays, light, eps):
    light = np.asarray(light, F).astype(np.float64); eps = float(F(eps))
    O, D = rays["O"].astype(np.float64), rays["D"].astype(np.float64)
    t = np.minimum(SHADOW_TMAX, rays["t"]).astype(np.float64)[:, None]
    tD = t * D
    I = O + tD; eI = U * np.abs(tD) + U * np.abs(I)
    L = light[None, :] - I; eL = eI + U * np.abs(L)
    Ld, eLd = _normalize64(L, eL)
    dist, edist = _length64(L, eL)
    Oo = I + Ld * eps
    eO = eI + (eps * eLd if eps else 0.0) + U * eps * np.abs(Ld) + U * np.abs(Oo)
    Dd, eD = _normalize64(Ld, eLd)
    tm = dist - eps
    return {"O": Oo, "eO": eO, "D": Dd, "eD": eD, "t": tm, "et": edist + U * np.abs(tm)}


# ---- comparing -----------------------------------------------------------------------------------------------------------------------------

def excess(got, want, bound):
    """max over components of (|got - want| - bound): <= 0 when inside.  Also returns the largest |got - want|."""
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(got, np.float64) - want)
        over = np.where(np.isinf(bound), -np.inf, d - bound)
    over = np.where(np.isnan(d), np.inf, over)
    return (float(over.max()) if over.size else -np.inf), (float(np.where(np.isinf(bound), 0.0, d).max()) if d.size else 0.0)


def ulp_distance(a, b):
    """Largest distance in float32 ulps between two arrays (0 = bit-equal up to the sign of zero)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    return int(d.max()) if d.size else 0


# ---- the ray-bin key -----------------------------------------------------------------------------------------------------------------------

def morton3(cx, cy, cz, bits):
    """x, y, z interleaved from bit 0: bit j of x lands on bit 3 j, of y on 3 j + 1, of z on 3 j + 2."""
    cx, cy, cz = (np.asarray(c, np.uint32) for c in (cx, cy, cz))
    code = np.zeros(cx.shape, np.uint32)
    for j in range(bits):
        for axis, c in enumerate((cx, cy, cz)):
            code |= ((c >> np.uint32(j)) & np.uint32(1)) << np.uint32(3 * j + axis)
    return code


def bin_cells(O, bounds6, cell_bits):
    """(n, 3) uint32: cell = uint32( fmin( fmax( (O - lo) * scale, 0 ), 2^b - 1 ) ), scale = float32( 2^b ) / (hi - lo), or 0 where the
    extent is not positive.  fmax / fmin drop a NaN, as fmaxf / fminf do."""
    O = np.asarray(O, F)
    b6 = np.asarray(bounds6, F)
    lo, ext = b6[:3], b6[3:] - b6[:3]
    with np.errstate(all="ignore"):
        scale = np.where(ext > 0, F(1 << cell_bits) / np.where(ext > 0, ext, F(1)), F(0)).astype(F)
        f = (O - lo[None, :]) * scale[None, :]
        assert f.dtype == F
        return np.fmin(np.fmax(f, F(0)), F((1 << cell_bits) - 1)).astype(np.uint32)


def bin_keys(rays, bounds6, cell_bits, flags):
    c = bin_cells(rays["O"], bounds6, cell_bits)
    cell = morton3(c[:, 0], c[:, 1], c[:, 2], cell_bits)
    D = rays["D"]
    octant = ((D[:, 0] < 0).astype(np.uint32) << np.uint32(2)) | ((D[:, 1] < 0).astype(np.uint32) << np.uint32(1)) | (D[:, 2] < 0).astype(np.uint32)
    if flags == 0:
        return cell
    if flags == 1:
        return (cell << np.uint32(3)) | octant
    assert flags == 2
    return (octant << np.uint32(3 * cell_bits)) | cell


def bin_count(cell_bits, flags):
    return 1 << (3 * cell_bits + (3 if flags else 0))


# ---- the inputs test_raygen_host.py and test_raygen_gpu.py share ---------------------------------------------------------------------------

def make_camera(eye, p1, p2, p3, width, height, spp_x, spp_y):
    from tinybvh_amd import Camera
    cam = Camera()
    cam.eye[:] = eye; cam.p1[:] = p1; cam.p2[:] = p2; cam.p3[:] = p3
    cam.width, cam.height, cam.spp_x, cam.spp_y = width, height, spp_x, spp_y
    return cam


def oblique_camera(width, height, spp_x, spp_y):
    """Nothing aligned with anything: every term of P = p1 + u (p2 - p1) + v (p3 - p1) rounds."""
    return make_camera((-9.3, 5.21, 4.87), (-7.41, 6.13, 3.75), (-7.29, 6.07, 5.93), (-7.53, 4.41, 3.81), width, height, spp_x, spp_y)


def symmetric_camera(width=64, height=32, spp_x=2, spp_y=2):
    """The pyramid centred on the z axis: the sample column at u = 1/2 has D.x == 0 exactly, the sample row at v = 1/2 D.y == 0."""
    return make_camera((0.0, 0.0, -3.0), (-1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (-1.0, -1.0, 0.0), width, height, spp_x, spp_y)


def negative_zero_camera(width=8, height=8, spp_x=1, spp_y=1):
    """p1.x = -0.0 with p2.x, p3.x < 0 and eye.x = +0.0: ray 0 (u = v = 0) has P.x = -0 + 0 * neg + 0 * neg = -0 and D.x = -0.0."""
    return make_camera((0.0, 0.0, 0.0), (-0.0, 1.0, 2.0), (-2.0, 1.0, 2.0), (-1.0, -1.0, 2.0), width, height, spp_x, spp_y)


# (scene golden, eye, view, width, height): the primary batches whose traced records feed the bounce and shadow generators.  The first looks
# into the triangle soup from outside (hits from both sides of triangles, misses through the gaps), the second along the atrium's floor
# and over its edge.
TRACED_VIEWS = {
    "soup_2k": ((-9.0, 5.2, 4.9), (1.0, 0.02, 0.03), 128, 96),
    "atrium_6k": ((-30.0, 6.0, 2.0), (0.9, -0.35, -0.1), 128, 64),
}
BOUNCE_SEEDS = (5, 0x9E3779B9)
SHADOW_LIGHT = (3.25, 12.5, 4.75)
SHADOW_EPS = 4e-5


def traced_view_rays(name):
    """The primary batch of TRACED_VIEWS[name], untraced (1 sample per pixel; host generator)."""
    from tinybvh_amd import rays as R
    eye, view, w, h = TRACED_VIEWS[name]
    return R.primary(R.camera(eye, view, w, h, 1, 1))


# name -> (camera, first, n): every case at most 8192 rays
def primary_cases():
    return {
        "spp2x2": (oblique_camera(64, 32, 2, 2), 0, 8192),
        "spp1x1": (oblique_camera(64, 32, 1, 1), 0, 2048),
        "spp3x2": (oblique_camera(64, 32, 3, 2), 64 * 32 * 6 - 8192, 8192),      # (not a power of two; the image's last 8192 rays)
        "one_tile_column": (oblique_camera(4, 64, 2, 2), 0, 1024),
        "odd_slice": (oblique_camera(64, 32, 2, 2), 16 * 4 * 3 + 7, 1001),        # first no multiple of 16 spp, n no multiple of 256
        "symmetric": (symmetric_camera(), 0, 8192),
        "negative_zero": (negative_zero_camera(), 0, 64),
        "index_above_2_32": (oblique_camera(65536, 65536, 2, 2), 2 ** 34 - 4096, 4096),
    }


def compare_f64(got, ref, label=""):
    """Hold records to a *_f64 reference: O, D and t inside their bounds, ray by ray; a bounce ray on a knife edge may instead be the
    ray with R reversed.  Asserts, and returns the figures (largest distances, in absolute terms and as a share of the bound)."""
    n = got.shape[0]

    def inside(suffix):
        ok = np.ones(n, bool); dist = {}
        for f in ("O", "D"):
            d = np.abs(got[f].astype(np.float64) - ref[f + suffix]); b = ref["e" + f + suffix]
            ok &= (((d <= b) | np.isinf(b)) & ~np.isnan(d)).all(axis=1)
            dist[f] = (d, b)
        return ok, dist

    main, dist = inside("")
    ok = main.copy()
    knife = ref.get("knife", np.zeros(n, bool))
    if knife.any():
        ok |= knife & inside("_alt")[0]
    with np.errstate(invalid="ignore"):
        dt = np.abs(got["t"].astype(np.float64) - ref["t"])
    t_ok = (dt <= ref["et"]) | np.isinf(ref["et"])
    fig = {"n": n, "knife": int(knife.sum()), "knife_reversed": int((knife & ~main & ok).sum()), "outside": int((~ok).sum()), "t_outside": int((~t_ok).sum())}
    for f, (d, b) in dist.items():
        sel = main[:, None] & np.isfinite(b) & (b > 0)
        fig["max_abs_" + f] = float(d[np.broadcast_to(main[:, None], d.shape) & np.isfinite(b)].max(initial=0.0))
        fig["max_share_" + f] = float((d[sel] / b[sel]).max(initial=0.0))
    sel = np.isfinite(ref["et"]) & (ref["et"] > 0)
    fig["max_abs_t"] = float(dt[sel].max(initial=0.0)); fig["max_share_t"] = float((dt[sel] / ref["et"][sel]).max(initial=0.0))
    print("f64", label, fig)
    assert fig["outside"] == 0 and fig["t_outside"] == 0, (label, fig)
    assert fig["knife"] <= KNIFE_CAP * n, (label, fig)
    return fig
