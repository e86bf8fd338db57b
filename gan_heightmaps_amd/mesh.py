"""Terrain as adaptive triangle meshes: a right-triangulated irregular network built on the device (csrc/mesh.hip).

What an engine loads is a mesh, and a heightmap triangulated pixel by pixel is nearly all triangles on ground a hundred would
describe.  ``ErrorMap`` gives every grid vertex an error once; ``extract`` then cuts a mesh at any tolerance: few triangles
where the land is smooth, many where it is not.  (RTIN: Evans, Kirkpatrick and Townsend 2001; "martini": Agafonkin 2019.)

The grid is a float32 height plane p of (R T + 1) x (C T + 1) vertices, T = 2^k the ``tile`` (1 <= k <= 12): a forest of R x C
root squares.  Every root square is split along its main diagonal (0, 0) - (T, T) in (row, col); a triangle (a, b, c) with
hypotenuse a - b and midpoint m splits into (c, a, m) and (b, c, m).  Every vertex that is no tile corner is the hypotenuse
midpoint of one or two triangles at exactly one scale s = min(tz(row), tz(col)) (tz: trailing zeros; coordinates modulo T),
d = 2^s, and

    err[m] = max(|(p[a] + p[b]) 0.5 - p[m]|, err of m's child midpoints),      err = +inf at the tiles' corners,

every operation rounded on its own in float32.  An *axis midpoint* (tz(row) != tz(col)) has its endpoints at +-d along the
axis with the smaller tz and the four children (+-d/2, +-d/2) (none at s = 0).  A *centre* (tz(row) = tz(col)) has as
endpoints two opposite corners of its 2d-square -- on the main diagonal when s = k - 1 or the square's index (Y, X) has an
even sum, on the anti-diagonal otherwise -- and the children (+-d, 0), (0, +-d).  Children outside the plane are skipped; a
vertex on the border between two tiles takes children from both sides, which is what makes the forest free of cracks.

The mesh at the tolerance ``max_error`` >= 0 (height units, strict > as in martini): the apex of a triangle is its parent's
midpoint and errors only grow upwards, so the triangle (a, b, apex) of the midpoint m is in the mesh iff err[apex] >
max_error >= err[m]; an axis midpoint of scale 0 above the tolerance gives the two unit halves of each of its triangles that
exist.  A vertex is used iff err > max_error.  Used vertices are numbered in row-major order; triangles are ordered by their
owning midpoint in row-major order, then by apex (the smaller row, in the same row the smaller column, first), the half at a
before the half at b; corners are (a, b, apex) or (a | b, m, apex) with the last two swapped where needed so that
(q - p) x (r - p) > 0 in (col, row) for every triangle (p, q, r).

The errors of a tile's vertices, its border included, depend on heights at most T - 2 pixels outside the tile.  An error map
over a rectangle grown by one ring of tiles therefore holds, on the inner tiles, the errors of the unbounded forest, and two
meshes cut from tile-aligned rectangles of one world (``TerrainWorld.mesh``) agree vertex for vertex on their common border.

    python -m gan_heightmaps_amd.mesh IN OUT.{glb,obj,npz} [--texture F] [--max-error E] [--tile T] [--height-scale S]
        [--plain | --fused]
"""
import argparse
import collections
import dataclasses
import functools
import json
import os
import struct
import sys

import numpy as np

from .planes import as_plane, scratch
from .util import form_choice, is_int as _is_int, is_number as _is_number, read_image

__all__ = ["DEFAULT_FUSED", "MAX_TILE", "DevicePlane", "ErrorMap", "TerrainMesh", "fit", "default_tile", "heightmap_mesh",
           "parse_args", "main"]

MAX_TILE = 1 << 12           # GHM_MESH_MAX_TILE_LOG2 (include/ghm.h)
# the form ``ErrorMap`` runs by default: the one tools/mesh_bench.py shows faster on the MI355X -- the plain one, 0.176
# against 0.301 ms for a 4097 x 4097 plane with tile 256 (DESIGN §4s has the line); both give the same bits
DEFAULT_FUSED = False

# a height plane that is on the device already: fp32 [rows, cols], contiguous
DevicePlane = collections.namedtuple("DevicePlane", "ptr rows cols")


def _tile_log2(tile):
    if not _is_int(tile) or tile < 2 or tile > MAX_TILE or tile & (tile - 1):
        raise ValueError("tile must be a power of two in [2, %d], got %r" % (MAX_TILE, tile))
    return int(tile).bit_length() - 1


def _check_error(max_error):
    if not _is_number(max_error) or max_error < 0 or not np.float32(max_error) < np.float32(3.4e38):
        raise ValueError("max_error must be a finite number >= 0, got %r" % (max_error,))
    return float(max_error)


def _check_scale(height_scale):
    if not _is_number(height_scale):
        raise ValueError("height_scale must be a finite number, got %r" % (height_scale,))
    return float(height_scale)


_plane = functools.partial(as_plane, unit_range=True)


def default_tile(rows, cols):
    """the largest power of two <= 256 that does not exceed the shorter side"""
    side = min(int(rows), int(cols))
    if side < 2:
        raise ValueError("a heightmap of %d x %d is too small for a mesh (2 x 2 at least)" % (rows, cols))
    return min(256, 1 << (side.bit_length() - 1))


def fit(heightmap, tile):
    """a host array (H, W) edge-replicated to the next (R tile + 1, C tile + 1) -> (array, (H, W)).  A 512 x 512 generator
    output becomes 513 x 513; the replicated strip is flat along its direction, has zero error and costs nothing."""
    _tile_log2(tile)
    a = np.asarray(heightmap)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("heightmap must be (H, W), got %s" % (a.shape,))
    H, W = a.shape
    rows = max(1, -(-(H - 1) // tile)) * tile + 1
    cols = max(1, -(-(W - 1) // tile)) * tile + 1
    if (rows, cols) != (H, W):
        a = np.pad(a, ((0, rows - H), (0, cols - W)), mode="edge")
    return np.ascontiguousarray(a), (H, W)


@dataclasses.dataclass(frozen=True, eq=False)
class TerrainMesh:
    """A mesh cut from an error map.  grid: int32 [V, 2], the (row, col) of each vertex inside ``shape`` = (rows, cols) of
    the meshed rectangle; heights: float32 [V]; triangles: uint32 [F, 3]; origin: the (row, col) of the rectangle's first
    vertex in whatever larger frame it was cut from (a world's pixel coordinates); valid_shape: the (H, W) of the part of
    ``shape`` that holds data (the rest is ``fit``'s padding), what the texture covers."""
    grid: np.ndarray
    heights: np.ndarray
    triangles: np.ndarray
    shape: tuple
    origin: tuple
    tile: int
    max_error: float
    valid_shape: tuple

    @property
    def vertices(self):
        return len(self.heights)

    @property
    def faces(self):
        return len(self.triangles)

    def positions(self, height_scale=64.0):
        """float32 [V, 3]: (origin_x + col, height_scale h, origin_y + row); y is up"""
        hs = np.float32(_check_scale(height_scale))
        p = np.empty((len(self.heights), 3), np.float32)
        p[:, 0] = (self.grid[:, 1].astype(np.int64) + self.origin[1]).astype(np.float32)
        p[:, 1] = hs * self.heights
        p[:, 2] = (self.grid[:, 0].astype(np.int64) + self.origin[0]).astype(np.float32)
        return p

    def uvs(self):
        """float32 [V, 2]: ((col + 0.5) / W, (row + 0.5) / H) over valid_shape, clamped to [0, 1]; v runs down the rows"""
        H, W = self.valid_shape
        uv = np.empty((len(self.heights), 2), np.float64)
        uv[:, 0] = (self.grid[:, 1] + 0.5) / W
        uv[:, 1] = (self.grid[:, 0] + 0.5) / H
        return np.clip(uv, 0.0, 1.0).astype(np.float32)

    def front_faces(self):
        """the triangles wound counter-clockwise seen from above (+y), as glTF and OBJ want their front faces: the canonical
        winding, positive in (col, row), looks down"""
        return np.ascontiguousarray(self.triangles[:, [0, 2, 1]])

    def save(self, path, texture=None, height_scale=64.0, instances=None):
        """write the mesh: .glb (binary glTF 2.0: one mesh, POSITION with min / max, TEXCOORD_0, uint32 indices; the texture
        embedded as a PNG), .obj (with .mtl and the texture's .png beside it when a texture is given) or .npz (the arrays).
        texture: uint8 (H, W, 3) or (H, W).  instances: a scatter.Scatter whose points lie in this mesh's frame (.glb only): one
        more node per species, a four-sided cone as a proxy mesh, placed by EXT_mesh_gpu_instancing's TRANSLATION, ROTATION
        and SCALE accessors in ``positions``' convention -- (col, height_scale h, row), the yaw about +y; without it the file
        is byte for byte what it was before instances existed."""
        ext = os.path.splitext(path)[1].lower()
        if ext not in (".glb", ".obj", ".npz"):
            raise ValueError("a mesh is written as .glb, .obj or .npz, got %r" % (path,))
        if texture is not None:
            texture = np.asarray(texture)
            if texture.dtype != np.uint8 or not (texture.ndim == 2 or (texture.ndim == 3 and texture.shape[2] == 3)):
                raise ValueError("texture must be uint8 (H, W, 3) or (H, W), got %s %s" % (texture.dtype, texture.shape))
        _check_scale(height_scale)
        if instances is not None and (ext != ".glb" or not hasattr(instances, "layers")):
            raise ValueError("instances go into a .glb and are a scatter.Scatter, got %r for %r" % (instances, path))
        if ext == ".npz":
            extra = {} if texture is None else {"texture": texture}
            np.savez(path, grid=self.grid, heights=self.heights, triangles=self.triangles, shape=np.asarray(self.shape),
                     origin=np.asarray(self.origin), tile=self.tile, max_error=self.max_error,
                     valid_shape=np.asarray(self.valid_shape), **extra)
        elif ext == ".glb":
            with open(path, "wb") as f:
                f.write(_glb(self, texture, height_scale, instances))
        else:
            _write_obj(self, path, texture, height_scale)
        return path


def _png_bytes(texture):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(texture).save(buf, format="PNG")
    return buf.getvalue()


def _glb(mesh, texture, height_scale, instances=None):
    pos, uv, idx = mesh.positions(height_scale), mesh.uvs(), mesh.front_faces()
    parts, views = [], []

    def view(data, target=None):
        off = sum(len(p) for p in parts)
        parts.append(data + b"\0" * (-len(data) % 4))
        v = {"buffer": 0, "byteOffset": off, "byteLength": len(data)}
        if target is not None:
            v["target"] = target
        views.append(v)
        return len(views) - 1
    accessors = [
        {"bufferView": view(pos.tobytes(), 34962), "componentType": 5126, "count": len(pos), "type": "VEC3",
         "min": [float(v) for v in pos.min(0)] if len(pos) else [0.0] * 3,
         "max": [float(v) for v in pos.max(0)] if len(pos) else [0.0] * 3},
        {"bufferView": view(uv.tobytes(), 34962), "componentType": 5126, "count": len(uv), "type": "VEC2"},
        {"bufferView": view(idx.tobytes(), 34963), "componentType": 5125, "count": int(idx.size), "type": "SCALAR"}]
    prim = {"attributes": {"POSITION": 0, "TEXCOORD_0": 1}, "indices": 2, "mode": 4}
    doc = {"asset": {"version": "2.0", "generator": "gan_heightmaps_amd.mesh"}, "scene": 0, "scenes": [{"nodes": [0]}],
           "nodes": [{"mesh": 0, "name": "terrain"}], "meshes": [{"primitives": [prim], "name": "terrain"}],
           "accessors": accessors}
    if texture is not None:
        img = view(_png_bytes(texture))
        prim["material"] = 0
        doc["materials"] = [{"name": "terrain", "doubleSided": True,
                             "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0,
                                                      "roughnessFactor": 1.0}}]
        doc["textures"] = [{"source": 0, "sampler": 0}]
        doc["samplers"] = [{"magFilter": 9729, "minFilter": 9987, "wrapS": 33071, "wrapT": 33071}]
        doc["images"] = [{"bufferView": img, "mimeType": "image/png"}]
    if instances is not None:
        _glb_instances(doc, accessors, view, instances, height_scale)
    doc["bufferViews"] = views
    binary = b"".join(parts)
    doc["buffers"] = [{"byteLength": len(binary)}]
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    total = 12 + 8 + len(text) + 8 + len(binary)
    return b"".join((struct.pack("<4sII", b"glTF", 2, total), struct.pack("<I4s", len(text), b"JSON"), text,
                     struct.pack("<I4s", len(binary), b"BIN\0"), binary))


# the proxy of an instance: a cone of height 1 on a square base of side 1 around the origin, faces counter-clockwise from outside
_CONE = (np.array([[-0.5, 0, -0.5], [0.5, 0, -0.5], [0.5, 0, 0.5], [-0.5, 0, 0.5], [0, 1, 0]], np.float32),
         np.array([[0, 4, 1], [1, 4, 2], [2, 4, 3], [3, 4, 0], [0, 1, 2], [0, 2, 3]], np.uint16))


def _glb_instances(doc, accessors, view, instances, height_scale):
    """one node per layer of the Scatter: the cone, instanced by EXT_mesh_gpu_instancing"""
    hs = np.float32(height_scale)
    cone, faces = _CONE
    accessors.append({"bufferView": view(cone.tobytes(), 34962), "componentType": 5126, "count": len(cone), "type": "VEC3",
                      "min": [-0.5, 0.0, -0.5], "max": [0.5, 1.0, 0.5]})
    accessors.append({"bufferView": view(faces.tobytes(), 34963), "componentType": 5123, "count": int(faces.size), "type": "SCALAR"})
    doc["meshes"].append({"primitives": [{"attributes": {"POSITION": len(accessors) - 2}, "indices": len(accessors) - 1,
                                          "mode": 4}], "name": "cone"})
    doc["extensionsUsed"] = ["EXT_mesh_gpu_instancing"]
    for layer in instances.layers:
        n = len(layer)
        if n == 0:                      # an accessor holds at least one element: a species without points gets no node
            continue
        tr = np.empty((n, 3), np.float32)
        tr[:, 0] = layer.points[:, 1].astype(np.float32)
        tr[:, 1] = hs * layer.height
        tr[:, 2] = layer.points[:, 0].astype(np.float32)
        half = layer.yaw.astype(np.float64) / 2
        rot = np.zeros((n, 4), np.float32)
        rot[:, 1], rot[:, 3] = np.sin(half), np.cos(half)
        sc = np.repeat(layer.scale.astype(np.float32)[:, None], 3, axis=1)
        attrs = {}
        for key, data, kind in (("TRANSLATION", tr, "VEC3"), ("ROTATION", rot, "VEC4"), ("SCALE", sc, "VEC3")):
            accessors.append({"bufferView": view(np.ascontiguousarray(data).tobytes()), "componentType": 5126, "count": n,
                              "type": kind})
            attrs[key] = len(accessors) - 1
        doc["nodes"].append({"mesh": 1, "name": layer.species.name, "extensions": {"EXT_mesh_gpu_instancing": {"attributes": attrs}}})
        doc["scenes"][0]["nodes"].append(len(doc["nodes"]) - 1)


def _write_obj(mesh, path, texture, height_scale):
    pos, uv, idx = mesh.positions(height_scale), mesh.uvs(), mesh.front_faces().astype(np.int64) + 1
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    with open(path, "w") as f:
        f.write("# gan_heightmaps_amd.mesh: %d vertices, %d triangles, max_error %r\n" % (len(pos), len(idx), mesh.max_error))
        if texture is not None:
            f.write("mtllib %s.mtl\nusemtl terrain\n" % name)
        f.write("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in pos))
        f.write("".join("vt %r %r\n" % (float(u), 1.0 - float(v)) for u, v in uv))         # OBJ's v runs up
        f.write("".join("f %d/%d %d/%d %d/%d\n" % (a, a, b, b, c, c) for a, b, c in idx))
    if texture is not None:
        with open(stem + ".mtl", "w") as f:
            f.write("newmtl terrain\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nmap_Kd %s.png\n" % name)
        with open(stem + ".png", "wb") as f:
            f.write(_png_bytes(texture))


class ErrorMap:
    """The error of every vertex of a height plane, kept on the device: one map serves any number of tolerances (an engine's
    LOD chain).  ops: a device.Ops; heightmap: a host array (R tile + 1, C tile + 1) (see ``fit``), uint8 or floating point in
    [0, 1] -- or a DevicePlane(ptr, rows, cols), fp32 and contiguous, which the map frees on close() when ``own``.  fused:
    the LDS form of the finest scales (True) or one launch per sub-level (False): the same bits; default DEFAULT_FUSED.
    origin, valid_shape: handed on to the meshes.  A context manager; close() frees the device planes."""

    def __init__(self, ops, heightmap, tile=256, fused=None, origin=(0, 0), valid_shape=None, own=True):
        self.tile, self._k = int(tile), _tile_log2(tile)
        self.fused = DEFAULT_FUSED if fused is None else bool(fused)
        plane = heightmap if isinstance(heightmap, DevicePlane) else _plane(heightmap)
        rows, cols = (plane.rows, plane.cols) if isinstance(plane, DevicePlane) else plane.shape
        T = self.tile
        if rows <= T or cols <= T or (rows - 1) % T or (cols - 1) % T:
            raise ValueError("a plane of %d x %d is not (R tile + 1) x (C tile + 1) for tile = %d (see mesh.fit)" % (rows, cols, T))
        if rows * cols >= 1 << 31:
            raise ValueError("a plane of %d x %d is at or beyond 2^31 vertices" % (rows, cols))
        self.rows, self.cols = int(rows), int(cols)
        self.origin = (int(origin[0]), int(origin[1]))
        self.valid_shape = (self.rows, self.cols) if valid_shape is None else (int(valid_shape[0]), int(valid_shape[1]))
        self._ops, self._dev = ops, ops.dev
        self._src = self._err = None
        self._own = True
        dev = self._dev
        try:
            if isinstance(plane, DevicePlane):
                self._src, self._own = plane.ptr, bool(own)
            else:
                self._src = dev.alloc(plane.nbytes)
                dev.h2d(self._src, plane)
            self._err = dev.alloc(4 * self.rows * self.cols)
            ops.mesh_errors(self._src, self.rows, self.cols, self.cols, self._k, self.fused, self._err, self.cols)
        except Exception:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        dev = self._dev
        if self._src is None and self._err is None:
            return
        dev.sync()
        if self._src is not None and self._own:
            dev.free(self._src)
        if self._err is not None:
            dev.free(self._err)
        self._src = self._err = None

    def _open(self):
        if self._err is None:
            raise ValueError("this ErrorMap is closed")

    def errors(self):
        """the error plane, float32 [rows, cols], +inf at the tiles' corners"""
        self._open()
        out = np.empty((self.rows, self.cols), np.float32)
        self._dev.sync()
        self._dev.d2h(out, self._err, out.nbytes)
        return out

    def _rect(self, rect):
        if rect is None:
            return 0, 0, self.rows - 1, self.cols - 1
        try:
            y0, x0, h, w = rect
        except (TypeError, ValueError):
            raise ValueError("rect must be (y0, x0, h, w), got %r" % (rect,))
        T = self.tile
        if not all(_is_int(v) for v in (y0, x0, h, w)) or y0 < 0 or x0 < 0 or h < T or w < T or y0 % T or x0 % T or h % T \
                or w % T or y0 + h > self.rows - 1 or x0 + w > self.cols - 1:
            raise ValueError("rect %r is not a rectangle of whole tiles of %d inside the plane of %d x %d vertices"
                             % (tuple(rect), T, self.rows, self.cols))
        return int(y0), int(x0), int(h), int(w)

    def _count(self, tol, rect, ws):
        y0, x0, h, w = rect
        return self._ops.mesh_count(self._err, self.rows, self.cols, self.cols, self._k, y0, x0, h, w, tol, ws)

    def count(self, max_error, rect=None):
        """(V, F) of the mesh at this tolerance; nothing but the blocks' sums is written"""
        self._open()
        tol, rect = _check_error(max_error), self._rect(rect)
        with scratch(self._dev) as alloc:
            return self._count(tol, rect, alloc(self._ops.mesh_workspace(rect[2], rect[3])))

    def extract(self, max_error, rect=None):
        """the mesh at this tolerance as a TerrainMesh; rect = (y0, x0, h, w): the tiles [y0, y0 + h] x [x0, x0 + w] of the
        plane only (multiples of the tile), the mesh's origin moved there"""
        self._open()
        tol, rect = _check_error(max_error), self._rect(rect)
        y0, x0, h, w = rect
        dev, ops = self._dev, self._ops
        with scratch(dev) as scr:
            def alloc(n):                                         # (an empty mesh still gets pointers)
                return scr(max(int(n), 4))
            ws = alloc(ops.mesh_workspace(h, w))
            V, F = self._count(tol, rect, ws)
            grid, heights, tris = np.empty((V, 2), np.int32), np.empty(V, np.float32), np.empty((F, 3), np.uint32)
            index, d_grid, d_heights, d_tris = alloc(4 * (h + 1) * (w + 1)), alloc(8 * V), alloc(4 * V), alloc(12 * F)
            ops.mesh_extract(self._src, self.cols, self._err, self.rows, self.cols, self.cols, self._k, y0, x0, h, w, tol, ws,
                             index, d_grid, d_heights, d_tris, V, F)
            dev.sync()
            for host, ptr in ((grid, d_grid), (heights, d_heights), (tris, d_tris)):
                if host.nbytes:
                    dev.d2h(host, ptr, host.nbytes)
        vh, vw = self.valid_shape
        valid = (max(1, min(h + 1, vh - y0)), max(1, min(w + 1, vw - x0)))
        return TerrainMesh(grid, heights, tris, (h + 1, w + 1), (self.origin[0] + y0, self.origin[1] + x0), self.tile, tol,
                           valid)


def heightmap_mesh(ops, heightmap, max_error, tile=None, fused=None):
    """fit, build the error map and extract: the mesh of a heightmap of any size.  heightmap: (H, W) or (1, H, W), uint8 or
    floating point in [0, 1]; tile: None means default_tile(H, W)"""
    tol = _check_error(max_error)
    a = _plane(heightmap)
    tile = default_tile(*a.shape) if tile is None else tile
    plane, valid = fit(a, tile)
    with ErrorMap(ops, plane, tile=tile, fused=fused, valid_shape=valid) as em:
        return em.extract(tol)


# ---- command line -------------------------------------------------------------------------------------------------------
def _positive_tile(p, tile):
    try:
        _tile_log2(tile)
    except ValueError as e:
        p.error(str(e))


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.mesh",
                                description="Turn a heightmap into an adaptive triangle mesh (a RTIN cut on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("output", help="the mesh: .glb (binary glTF 2.0), .obj or .npz")
    p.add_argument("--texture", default=None, metavar="F", help="an image of the heightmap's size to drape over the mesh")
    p.add_argument("--max-error", type=float, default=0.01, help="tolerance in height units (heights are in [0, 1]; default 0.01)")
    p.add_argument("--tile", type=int, default=None, help="root square side, a power of two (default: the largest <= 256 that fits)")
    p.add_argument("--height-scale", type=float, default=64.0, help="pixels per unit height (default 64, the renderer's)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="one launch per sub-level")
    g.add_argument("--fused", action="store_true", help="the finest scales in one launch from LDS (the same bits)")
    a = p.parse_args(argv)
    if os.path.splitext(a.output)[1].lower() not in (".glb", ".obj", ".npz"):
        p.error("the output must be .glb, .obj or .npz")
    try:
        _check_error(a.max_error)
        _check_scale(a.height_scale)
    except ValueError as e:
        p.error(str(e))
    if a.tile is not None:
        _positive_tile(p, a.tile)
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    tex = None if a.texture is None else np.ascontiguousarray(read_image(a.texture, "RGB", mmap=False))
    dev = Device(0)
    try:
        m = heightmap_mesh(Ops(dev), x, a.max_error, tile=a.tile, fused=form_choice(a.fused, a.plain))
    finally:
        dev.close()
    m.save(a.output, texture=tex, height_scale=a.height_scale)
    print("%s: %d vertices, %d triangles (%.2f %% of %d)" % (a.output, m.vertices, m.faces,
                                                             100.0 * m.faces / max(1, 2 * (m.shape[0] - 1) * (m.shape[1] - 1)),
                                                             2 * (m.shape[0] - 1) * (m.shape[1] - 1)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
