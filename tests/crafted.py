"""Scenes built splat by splat, in pixels, for the compositor's edges (tests/test_crafted_scenes.py states on the CPU oracle that every scene IS what
it claims, tests/test_gpu_compositor_edges.py holds the HIP compositor to the oracle on them).

`asset()` generalises test_oracle.fp32_point_asset: an all-fp32, chunk-less asset (decode is the identity) with per-splat position, scale, rotation (the
10-10-10-2 smallest-three packing), RGB and opacity.  `PixelCamera` turns "a splat centred on pixel (x, y) at view depth d with a footprint of sigma pixels"
into object-space numbers: the camera sits on +z and looks down -z with y up, so object x / y / z are screen right / up / towards the camera, a splat's
x- and y-scales are its screen sigmas (an identity rotation; the needles turn about z) and its z-scale is kept at 1e-5 pixel: far off the axis the
perspective Jacobian leaks depth extent into the footprint (65,535-pixel targets put splats at |x / z| of a few thousand).

What a footprint is (RenderGaussianSplats.shader through the oracle's prepare()): the 2D covariance is sigma^2 + 0.3 per axis, an axis of the quad is
s = sqrt(2 lambda) pixels long, the quad reaches |q| <= 2 per axis, a fragment lives where saturate(exp(-|q|^2) * opacity) >= 1/255.  Hence the bricks:

  dot      sigma (0.30, 0.10), opacity 1.25/255, centred on a pixel centre: s = (0.88, 0.79), alpha at the neighbour pixel <= 0.28 * opacity < 1/255, so
           exactly ONE live fragment, of alpha == opacity (0.0049: a pixel under four of them stays below A = 0.02, nothing saturates, every record of
           a list is walked).  Sigmas differ on purpose: an exactly isotropic footprint has no eigenvector and the reference normalises (0, 0) to NaN.
  square   sigma 1.3038 (s = 2.0, the quad is the 8 x 8 pixels around its centre, +-0.49 pixel of margin), opacity 4000: exp(-|q|^2) * 4000 >= 8.7 on the
           whole quad, saturate() makes every fragment alpha == 1.0, so ONE blend puts A == 1.0 (fp16 0x3c00) on exactly one 8x8 quadrant."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import oracle_lib as O
from common import rt_diff
from unitygaussiansplatting_amd import asset as A
from unitygaussiansplatting_amd import camera, creator

TILE_SHAPES = ((16, 16), (32, 16), (32, 32))
DOT_SIGMA = (0.30, 0.10)
DOT_OPACITY = 1.25 / 255.0
SQUARE_SIGMA = math.sqrt(2.0 - 0.3)            # lambda = sigma^2 + 0.3 = 2 -> s = sqrt(2 lambda) = 2 pixels, the quad |q| <= 2 is +-4 pixels
SQUARE_OPACITY = 4000.0


def pack_rotation(q) -> np.ndarray:
    """Quaternions (n x 4, xyzw) -> the asset's 10-10-10-2 words (GaussianUtils.cs:46-76 + the Norm10 store)."""
    q = np.asarray(q, np.float64).reshape(-1, 4)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return creator.EncodeQuatToNorm10(creator.PackSmallest3Rotation(q)).astype(np.uint32)


def asset(pos, scale, rot=None, rgb=None, opacity=None) -> A.GaussianSplatAsset:
    """All-fp32, chunk-less asset: pos n x 3, scale n x 3 (object units), rot n x 4 quaternions xyzw (None = identity), rgb n x 3 (None = 0.5; not
    clamped anywhere), opacity n (None = 1; SH all zero, so the colour of the 40-byte view record is f16(rgb), f16(opacity))."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    other = np.zeros((n, 4), np.uint32)
    other[:, 0] = pack_rotation(np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if rot is None else rot)
    other[:, 1:4] = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float32), (n, 3))).view(np.uint32)
    w, h = A.CalcTextureSize(n)
    col = np.zeros((w * h, 4), np.float32)
    texel = creator.SplatIndexToTextureIndex(np.arange(n, dtype=np.uint32))          # the Morton-swizzled texel of splat i
    col[texel, :3] = 0.5 if rgb is None else np.asarray(rgb, np.float32).reshape(-1, 3)
    col[texel, 3] = 1.0 if opacity is None else np.asarray(opacity, np.float32).reshape(-1)
    return A.GaussianSplatAsset(splatCount=n, posFormat=A.VectorFormat.Float32, scaleFormat=A.VectorFormat.Float32, shFormat=A.SHFormat.Float32,
                                colorFormat=A.ColorFormat.Float32x4, posData=pos.view(np.uint8).reshape(-1).copy(),
                                otherData=other.view(np.uint8).reshape(-1).copy(), colorData=col.view(np.uint8).reshape(-1).copy(),
                                shData=np.zeros(n * 192, np.uint8))


class PixelCamera:
    """A camera on +z looking down -z at the origin, and the pixel <-> object-space arithmetic of its (W, H) target."""
    EYE_Z = 10.0

    def __init__(self, W: int, H: int, fov: float = 39.0965):
        self.W, self.H = int(W), int(H)
        self.cam = camera.Camera(position=(0.0, 0.0, self.EYE_Z), target=(0.0, 0.0, 0.0), pixelWidth=self.W, pixelHeight=self.H, fieldOfView=fov)
        self.focal = self.H / (2.0 * math.tan(math.radians(fov) * 0.5))            # pixels per unit of x / z (== W * proj[0][0] / 2)

    def place(self, px, py, depth) -> np.ndarray:
        """Object-space centres of splats that project to pixel coordinates (px, py) (pixel k's centre is k + 0.5, y down) at view depth `depth`."""
        px, py, d = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(depth, np.float64))
        return np.stack([(px - 0.5 * self.W) / self.focal * d, -(py - 0.5 * self.H) / self.focal * d, self.EYE_Z - d], axis=-1)

    def scale(self, sigma_x, sigma_y, depth) -> np.ndarray:
        """Object-space scales of splats whose unrotated footprint has standard deviations (sigma_x, sigma_y) pixels at view depth `depth`."""
        sx, sy, d = np.broadcast_arrays(np.asarray(sigma_x, np.float64), np.asarray(sigma_y, np.float64), np.asarray(depth, np.float64))
        return np.stack([sx * d / self.focal, sy * d / self.focal, 1.0e-5 * d / self.focal], axis=-1)


class Builder:
    """Collects splats stated in pixels; depth decides the draw order (nearest first: the blend is 'under')."""

    def __init__(self, W: int, H: int):
        self.pc = PixelCamera(W, H)
        self.rows = []

    def add(self, px, py, depth, sigma_x, sigma_y, rgb, opacity, angle=0.0) -> np.ndarray:
        """Vectorised; angle = counter-clockwise turn of the footprint about the view axis, radians.  Returns the indices of the splats added."""
        px = np.atleast_1d(np.asarray(px, np.float64))
        n = len(px)
        b = lambda v: np.broadcast_to(np.asarray(v, np.float64), (n,))
        ang = b(angle)
        q = np.stack([np.zeros(n), np.zeros(n), np.sin(0.5 * ang), np.cos(0.5 * ang)], 1)
        first = sum(len(r[0]) for r in self.rows)
        self.rows.append((self.pc.place(px, b(py), b(depth)), self.pc.scale(b(sigma_x), b(sigma_y), b(depth)), q,
                          np.broadcast_to(np.asarray(rgb, np.float64), (n, 3)), b(opacity)))
        return np.arange(first, first + n)

    def build(self) -> A.GaussianSplatAsset:
        cat = lambda k: np.concatenate([r[k] for r in self.rows])
        return asset(cat(0), cat(1), cat(2), cat(3), cat(4))


@dataclasses.dataclass
class Scene:
    name: str
    W: int
    H: int
    asset: A.GaussianSplatAsset
    meta: dict

    @functools.cached_property
    def cam(self) -> camera.Camera:
        return PixelCamera(self.W, self.H).cam


# ---- the oracle side of a scene, and the tests' own statement of what a tile list is ---------------------------------------------------------------
def oracle_frame(scene: Scene, deleted=None, blend: int = 0, rt=None, want_frame: bool = True, window=None):
    """(oracle after sort + calc_view, frame params, frame or None); `deleted` = splat indices whose deleted bit is set; `window` = (x0, y0, x1, y1)
    inclusive: only those pixels are composited."""
    orc = O.Oracle(scene.asset)
    tr = camera.Transform()
    cam = scene.cam
    orc.sort(camera.sort_matrix(cam, tr.localToWorldMatrix))
    P = camera.frame_params(cam, tr)
    bits = None
    if deleted is not None:
        m = np.zeros((scene.asset.splatCount + 31) // 32 * 32, np.uint8)
        m[np.asarray(deleted, np.int64)] = 1
        bits = np.packbits(m, bitorder="little").view(np.uint32)
    orc.calc_view(P, deleted_bits=bits)
    return orc, P, (orc.draw(P, blend, rt=rt, window=window) if want_frame else None)


def tile_rects(rects: np.ndarray, tile):
    """raster_records' rectangles (n x 2 u32: x0 | y0 << 16, (x1 + 1) | (y1 + 1) << 16, 0 = not drawn) -> (drawn, tx0, tx1, ty0, ty1), inclusive tiles."""
    tw, th = int(tile[0]), int(tile[1])
    lo, hi = rects[:, 0].astype(np.int64), rects[:, 1].astype(np.int64)
    drawn = hi != 0
    x0, y0, x1, y1 = lo & 0xffff, lo >> 16, (hi & 0xffff) - 1, (hi >> 16) - 1
    return drawn, x0 // tw, x1 // tw, y0 // th, y1 // th


def tile_lists(rects: np.ndarray, tile, W: int, H: int):
    """(list length of every tile, tilesY x tilesX; tiles per splat, n): a splat is on the list of every tile its pixel rectangle overlaps."""
    tw, th = int(tile[0]), int(tile[1])
    tilesX, tilesY = -(-W // tw), -(-H // th)
    drawn, tx0, tx1, ty0, ty1 = tile_rects(rects, tile)
    per_splat = np.where(drawn, (tx1 - tx0 + 1) * (ty1 - ty0 + 1), 0)
    d = np.zeros((tilesY + 1, tilesX + 1), np.int64)                      # a 2D difference array: +1 on the rectangle, summed up afterwards
    for sy, sx, sgn in ((ty0, tx0, 1), (ty0, tx1 + 1, -1), (ty1 + 1, tx0, -1), (ty1 + 1, tx1 + 1, 1)):
        np.add.at(d, (sy[drawn], sx[drawn]), sgn)
    lengths = d.cumsum(0).cumsum(1)[:tilesY, :tilesX]
    assert int(lengths.sum()) == int(per_splat.sum())
    return lengths, per_splat


def tile_list(rects: np.ndarray, order: np.ndarray, tile, tx: int, ty: int) -> np.ndarray:
    """The splats on tile (tx, ty)'s list, in draw order."""
    drawn, tx0, tx1, ty0, ty1 = tile_rects(rects, tile)
    on = drawn & (tx0 <= tx) & (tx <= tx1) & (ty0 <= ty) & (ty <= ty1)
    return order[on[order]]


def checked_tile_lists(scene: Scene, tile):
    """(oracle, frame params, rectangles) + tile_lists, with the total held against Oracle.pairs (the helper and the oracle's own count must agree)."""
    orc, P, _ = oracle_frame(scene, want_frame=False)
    _, rects, _ = orc.raster_records(P)
    lengths, per_splat = tile_lists(rects, tile, scene.W, scene.H)
    assert int(lengths.sum()) == orc.pairs(P, tile), (scene.name, tile)
    return orc, P, rects, lengths, per_splat


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------------------
def list_lengths_for(tile):
    nt = tile[0] * tile[1]                                                 # records per staging batch = threads of the blend's workgroup
    return [1, 63, 64, 65, nt - 1, nt, nt + 1, 2 * nt - 1, 2 * nt, 2 * nt + 1, 3 * nt + 1]


def _bright(rng, n):
    return rng.uniform(8.0, 24.0, (n, 3))       # a dot adds colour * 0.0049 * (1 - A): 0.04 .. 0.12 per channel, against the 2^-6 the premise asks for


@functools.lru_cache(maxsize=None)
def list_length_scene(tile) -> Scene:
    """One designed tile per length in list_lengths_for(tile), at tile (1 + 2k, 1), untouched tiles all around; the list of length L is L dots, record j of
    the list (depth order) on pixel perm_layer(j mod NT) of the tile: every record has one live fragment of its own, batches of NT records fill the tile
    once each, and the pixel a record lands on is not the thread that stages it."""
    tw, th = tile
    nt = tw * th
    lengths = list_lengths_for(tile)
    W, H = tw * (2 * len(lengths) + 1), th * 3
    b = Builder(W, H)
    rng = np.random.default_rng(tw * 100 + th)
    designed = {}
    depth0 = 4.0
    for k, L in enumerate(lengths):
        tx, ty = 1 + 2 * k, 1
        j = np.arange(L)
        layer, slot = j // nt, j % nt
        pix = (slot * 37 + 11 * (layer + 1) + 5 * k) % nt if L >= nt else (slot * (nt // 64 * 37 + 1) + 3 * k) % nt      # 37 is odd: a permutation of 0 .. NT-1
        assert len(np.unique(pix + layer * nt)) == L
        b.add(tx * tw + pix % tw + 0.5, ty * th + pix // tw + 0.5, depth0 + 1.0e-4 * j + 0.37 * k, DOT_SIGMA[0], DOT_SIGMA[1], _bright(rng, L), DOT_OPACITY)
        designed[(tx, ty)] = L
    return Scene(f"list_lengths_{tw}x{th}", W, H, b.build(), dict(tile=tile, designed=designed))


def quadrants_of(tile):
    return [(qx, qy) for qy in range(tile[1] // 8) for qx in range(tile[0] // 8)]


@functools.lru_cache(maxsize=None)
def early_termination_scene(tile) -> Scene:
    """Two designed tiles in a target whose size is no multiple of 8 in either direction: the interior tile (1, 1) and the bottom-right tile, of which
    only (tile_w - 11) x (tile_h - 3) pixels are inside (its rightmost column of 8x8 quadrants lies wholly outside the target, the next one has 5 pixels inside).  In each, list positions 0 .. NW-2 are squares that saturate every 8x8 quadrant but the `late`
    one; 2 NT + 5 dots follow, all behind the squares (they add exactly 0); the late quadrant's ONLY splats -- three soft ones -- come last, in the third
    staging batch.  A compositor that stops the tile once the early quadrants are done, or counts a pixel outside the target as unfinished, or takes a
    non-zero starting target for zero, is off by those three splats."""
    tw, th = tile
    nt = tw * th
    W, H = 3 * tw + (tw - 11), 2 * th + (th - 3)
    b = Builder(W, H)
    rng = np.random.default_rng(tw * 1000 + th)
    tiles = {}
    for which, (tx, ty) in (("interior", (1, 1)), ("edge", (3, 2))):
        x0, y0 = tx * tw, ty * th
        quads = [(qx, qy) for qx, qy in quadrants_of(tile) if x0 + 8 * qx < W and y0 + 8 * qy < H]        # quadrants with at least one pixel inside
        late = quads[1] if which == "interior" else quads[-1]                # the edge tile's late quadrant holds the target's last pixel (5 x 5 inside)
        early = [q for q in quads if q != late]
        depth = 3.0 + (0.0 if which == "interior" else 1.0)
        squares = b.add([x0 + 8 * qx + 4.0 for qx, _ in early], [y0 + 8 * qy + 4.0 for _, qy in early], depth + 1.0e-3 * np.arange(len(early)),
                        SQUARE_SIGMA, SQUARE_SIGMA * 1.02, rng.uniform(0.2, 1.0, (len(early), 3)), SQUARE_OPACITY)
        # filler dots on inside pixels of the early quadrants
        pix = np.array([(x0 + 8 * qx + i, y0 + 8 * qy + j) for qx, qy in early for j in range(8) for i in range(8) if x0 + 8 * qx + i < W and y0 + 8 * qy + j < H])
        nfill = 2 * nt + 5 - len(early)
        sel = pix[rng.integers(0, len(pix), nfill)]
        fill = b.add(sel[:, 0] + 0.5, sel[:, 1] + 0.5, depth + 0.1 + 1.0e-4 * np.arange(nfill), DOT_SIGMA[0], DOT_SIGMA[1], _bright(rng, nfill), DOT_OPACITY)
        # the late quadrant's splats: centred on the middle of its inside pixels, soft enough to stay within +-4 pixels (sigma 0.8: the quad reaches 2.97)
        lx0, ly0 = x0 + 8 * late[0], y0 + 8 * late[1]
        cx, cy = 0.5 * (lx0 + min(lx0 + 8, W)), 0.5 * (ly0 + min(ly0 + 8, H))
        lates = b.add([cx - 0.5, cx + 0.3, cx], [cy, cy - 0.4, cy + 0.5], depth + 0.5 + 1.0e-3 * np.arange(3), [0.8, 0.7, 0.6], [0.6, 0.8, 0.7],
                      [[1.0, 0.2, 0.1], [0.1, 1.0, 0.3], [0.2, 0.1, 1.0]], [0.55, 0.6, 0.5])
        tiles[which] = dict(tile=(tx, ty), early=early, late=late, squares=squares, fill=fill, lates=lates, batch=2)
    return Scene(f"early_termination_{tw}x{th}", W, H, b.build(), dict(tile=tile, tiles=tiles))


def grid_size(tiles_x: int, tiles_y: int, tile=(16, 16)):
    """A target of exactly tiles_x x tiles_y tiles whose last column and row are partial."""
    return tiles_x * tile[0] - 5, tiles_y * tile[1] - 9


# tile count -> (tiles_x, tiles_y) at 16x16, both sides of every class boundary of the pair sort's dispatch: digit widths 6 / 7 / 8 bits in one pass
# (<= 64, <= 128, <= 256 tiles), 6 / 7 / 8 bits in two (<= 4,096, <= 16,384, <= 65,536), three passes above; per-tile counters up to 2,048 tiles.
# 65,537 is prime (one row of it would be 1,048,592 pixels wide, the library takes 65,535): 65,538 = 198 x 331 is the smallest count above 65,536 that a
# target can have, its last two tile ids are the only ones that need a 17th bit.
GRID_CLASSES = {64: (8, 8), 65: (13, 5), 128: (16, 8), 129: (43, 3), 256: (16, 16), 257: (257, 1), 2048: (64, 32), 2049: (683, 3), 4096: (64, 64),
                4097: (17, 241), 16384: (128, 128), 16385: (145, 113), 65536: (256, 256), 65538: (198, 331), 131072: (256, 512)}


def grid_splats(num_tiles: int) -> int:
    """A few hundred splats; 20,000 on the largest grids, so that the two- and three-pass pair sorts run over several partitions of keys."""
    return 20_000 if num_tiles >= 65536 else 300


def pair_sort_passes(num_tiles: int) -> int:
    return 1 if num_tiles <= 256 else (2 if num_tiles <= 65536 else 3)


@functools.lru_cache(maxsize=None)
def grid_scene(W: int, H: int, n: int = 300) -> Scene:
    """n splats of 0.5 .. 6 pixels spread over the whole target, plus one of 2.5 pixels two pixels inside each corner (so tile 0 and the last tile id have
    pairs, and a 65,535-wide / -high target gets rectangles whose far corner is 65,535)."""
    b = Builder(W, H)
    rng = np.random.default_rng(W * 7 + H)
    sig = np.exp(rng.uniform(np.log(0.5), np.log(6.0), (n, 2)))
    b.add(rng.uniform(0, W, n), rng.uniform(0, H, n), rng.permutation(n) * 1.0e-3 + 3.0, sig[:, 0], sig[:, 1], rng.uniform(0.05, 1.0, (n, 3)),
          rng.uniform(0.2, 0.95, n), rng.uniform(0, np.pi, n))
    b.add([2.0, W - 2.0, 2.0, W - 2.0], [2.0, 2.0, H - 2.0, H - 2.0], 2.0 + 1.0e-3 * np.arange(4), 2.5, 2.0,
          [[1.0, 0.3, 0.2], [0.2, 1.0, 0.3], [0.3, 0.2, 1.0], [1.0, 1.0, 0.2]], 0.8)
    return Scene(f"grid_{W}x{H}_{n}", W, H, b.build(), dict(corners=np.arange(n, n + 4)))


HEAVY_SIZE = (640, 360)
HEAVY_LAYERS = 40


@functools.lru_cache(maxsize=None)
def heavy_tail_scene() -> Scene:
    """40 splats that each cover the whole 640 x 360 target (sigma 500 .. 900 pixels, opacity 0.03 .. 0.04: alpha >= 1/255 out to 1.4 s >= 990 pixels, so
    each is on EVERY tile's list; colour 3.0 in one channel, so that the deepest layer still adds 3 x 0.03 x (1 - A) > 2^-6 where A <= 0.8) interleaved in depth with 20,000 small ones (sigma 0.3 .. 1.2 pixels: most on one tile) and 300 needles (sigma 300 x 0.3 pixels = 1000 : 1, on
    the two diagonals: rectangles of hundreds of tiles with live fragments in a band two pixels wide), 60 of them centred up to 200 pixels outside the
    target (these: opacity 0.7 .. 0.9, colour 1.5 .. 3, so that the stretch of the band that reaches in shows on its own).  Depth of blending per pixel: 40 layers + a few: C(48, 3) x (2^-13)^3 x 230,400 pixels x 4 channels / 4 (three shifts of one sign) = 0.007
    expected pixels beyond 2^-9 from the fp16 rounding argument of common.rt_err, so the frame is held to RT_TOL with no rare allowance."""
    W, H = HEAVY_SIZE
    b = Builder(W, H)
    rng = np.random.default_rng(640360)
    n_small, n_needle = 20_000, 300
    depth = 3.0 + rng.permutation(HEAVY_LAYERS + n_small + n_needle) * 2.0e-4
    d_full, d_small, d_needle = np.split(depth, [HEAVY_LAYERS, HEAVY_LAYERS + n_small])
    full = b.add(rng.uniform(0, W, HEAVY_LAYERS), rng.uniform(0, H, HEAVY_LAYERS), d_full, rng.uniform(500, 900, HEAVY_LAYERS), rng.uniform(500, 900, HEAVY_LAYERS),
                 3.0 * np.eye(3)[np.arange(HEAVY_LAYERS) % 3], rng.uniform(0.03, 0.04, HEAVY_LAYERS), rng.uniform(0, np.pi, HEAVY_LAYERS))
    sig = np.exp(rng.uniform(np.log(0.3), np.log(1.2), (n_small, 2)))
    small = b.add(rng.uniform(0, W, n_small), rng.uniform(0, H, n_small), d_small, sig[:, 0], sig[:, 1], rng.uniform(0.0, 1.0, (n_small, 3)),
                  rng.uniform(0.1, 0.9, n_small), rng.uniform(0, np.pi, n_small))
    nx, ny = rng.uniform(0, W, n_needle), rng.uniform(0, H, n_needle)
    off = np.arange(n_needle) < 60
    side = rng.integers(0, 4, n_needle)
    out = rng.uniform(20, 200, n_needle)
    nx = np.where(off & (side == 0), -out, np.where(off & (side == 1), W + out, nx))
    ny = np.where(off & (side == 2), -out, np.where(off & (side == 3), H + out, ny))
    needle = b.add(nx, ny, d_needle, 300.0, 0.3, np.where(off[:, None], rng.uniform(1.5, 3.0, (n_needle, 3)), rng.uniform(0.2, 1.0, (n_needle, 3))),
                   np.where(off, rng.uniform(0.7, 0.9, n_needle), rng.uniform(0.3, 0.7, n_needle)),
                   np.where(rng.random(n_needle) < 0.5, 0.25, 0.75) * np.pi + rng.uniform(-0.05, 0.05, n_needle))
    return Scene("heavy_tail", W, H, b.build(), dict(full=full, small=small, needle=needle, offscreen=needle[:60]))


def f16_neighbours_of_alpha_threshold():
    """The two fp16 numbers around 1/255 (which is not one): (below, above)."""
    t = np.float16(1.0 / 255.0)
    lo, hi = (t, np.nextafter(t, np.float16(1))) if float(t) < 1.0 / 255.0 else (np.nextafter(t, np.float16(0)), t)
    assert float(lo) < 1.0 / 255.0 < float(hi)
    return float(lo), float(hi)


@functools.lru_cache(maxsize=None)
def values_scene() -> Scene:
    """One 96 x 64 frame of the values the random scenes never hold: opacity exactly 1.0 (alpha == 1.0 only at a pixel centre the splat is centred on),
    opacity == the fp16 number just below 1/255 (never drawn) and just above it (drawn exactly where exp() rounds to 1: the pixel it is centred on),
    colours of exactly 0 and far above 1 (300: nothing clamps a premultiplied colour), on dots, on soft 3-pixel splats and under / over each other."""
    W, H = 96, 64
    b = Builder(W, H)
    lo, hi = f16_neighbours_of_alpha_threshold()
    gx, gy = np.meshgrid(np.arange(4, W, 8), np.arange(4, H, 8))
    gx, gy = gx.reshape(-1).astype(np.float64), gy.reshape(-1).astype(np.float64)
    n = len(gx)                                                            # 96 cells of 8 x 8 pixels, four kinds in turn
    kind = np.arange(n) % 4
    below = b.add(gx[kind == 0] + 0.5, gy[kind == 0] + 0.5, 3.0, DOT_SIGMA[0], DOT_SIGMA[1], [300.0, 300.0, 300.0], lo)
    above = b.add(gx[kind == 1] + 0.5, gy[kind == 1] + 0.5, 3.1, DOT_SIGMA[0], DOT_SIGMA[1], [300.0, 150.0, 75.0], hi)
    m = kind == 2                                                          # opaque (1.0) soft splat, black, over a bright one: hides it only at its centre pixel
    black = b.add(gx[m] + 0.5, gy[m] + 0.5, 3.2, 1.2, 0.9, [0.0, 0.0, 0.0], 1.0)
    under = b.add(gx[m] + 0.5, gy[m] + 0.5, 3.3, 1.5, 1.4, [300.0, 20.0, 0.0], 1.0)
    m = kind == 3                                                          # bright, opacity 1.0, off the pixel centres, a black veil of 0.3 in front
    veil = b.add(gx[m] + 0.2, gy[m] + 0.7, 3.4, 1.4, 1.0, [0.0, 0.0, 0.0], 0.3)
    bright = b.add(gx[m] + 0.2, gy[m] + 0.7, 3.5, 1.0, 1.3, [0.0, 300.0, 1000.0], 1.0)
    return Scene("values", W, H, b.build(), dict(below=below, above=above, black=black, under=under, veil=veil, bright=bright, lo=lo, hi=hi))


def observable(scene: Scene, splats, full=None, blend: int = 0, window=None) -> np.ndarray:
    """For each splat index: the largest rt_diff between the full frame and the frame with that ONE splat deleted (the oracle's deleted bits); with a
    `window` (x0, y0, x1, y1, inclusive) only those pixels are drawn and compared (the large grids: a corner's neighbourhood instead of 33 M pixels)."""
    cut = (lambda f: f) if window is None else (lambda f: f[window[1]:window[3] + 1, window[0]:window[2] + 1])
    if full is None:
        full = oracle_frame(scene, blend=blend, window=window)[2]
    return np.array([float(rt_diff(cut(oracle_frame(scene, deleted=[int(s)], blend=blend, window=window)[2]), cut(full)).max()) for s in splats])


def needles_reaching_in(scene: Scene, recs: np.ndarray, splats, reach: float = 1.0, margin: float = 4.0) -> np.ndarray:
    """Those of `splats` whose long axis, out to `reach` axis lengths from the centre (alpha there >= opacity / e), passes at least `margin` pixels inside
    the target: geometry alone (centre and axes of the oracle's raster records), no frame involved."""
    f = recs[np.asarray(splats)].view(np.float32)
    c, a1, a2 = f[:, 0:2], f[:, 2:4], f[:, 4:6]
    long_axis = np.where((np.hypot(*a1.T) >= np.hypot(*a2.T))[:, None], a1, a2)
    t = np.linspace(-reach, reach, 401)
    pts = c[:, None, :] + t[None, :, None] * long_axis[:, None, :]
    inside = (pts[..., 0] >= margin) & (pts[..., 0] <= scene.W - margin) & (pts[..., 1] >= margin) & (pts[..., 1] <= scene.H - margin)
    return np.asarray(splats)[inside.any(axis=1)]
