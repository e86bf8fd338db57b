"""``Pix2Pix``: the reference's trainer surface (/root/reference/pix2pix.py:19-425) on the libghm backend.

Same constructor arguments, attributes (train_fn, loss_fn, gen_fn, gen_fn_det, z_fn, z_fn_det, dcgan, p2p, lr,
train_keys) and methods (save_model, load_model, train, generate_*); compiled functions take numpy float32
arrays and return lists of numpy scalars / arrays, synchronously.
Extra keyword arguments (device, comm, use_graph, seed, dtype) configure the MI355X backend; ``dtype`` is the
arithmetic of the convolution products: 'bf16x3' (default = the reference's floatX=float32 as six exact bf16 piece products
per multiply-add on the bf16 matrix cores: csrc/conv_split.hip, fp32-accurate, held to the fp32 parity bounds, 1.55x the speed),
'f32' (the same arithmetic on the fp32 matrix instruction v_mfma_f32_32x32x2_f32) or 'bf16' / 'f16' (operands rounded).
"""
import gzip
import os
import pickle
from time import time

import numpy as np

from . import init as _init
from . import layers as L
from .device import Device
from .step import GanStep, OPT_RULES, TRAIN_KEYS
from .updates import adam, shared, OptimizerSpec
from .util import convert_to_rgb, imsave, makedirs, plot_grid, writes as util_writes

floatX = _init.floatX


class _Py2CompatPickler(pickle._Pickler):
    """numpy >= 2 pickles an ndarray through the global ``numpy._core.multiarray._reconstruct``; the reference's
    environment (Python 2, numpy <= 1.16) only has ``numpy.core.multiarray``, which every numpy up to 2.x still
    resolves.  Write that spelling so a checkpoint saved here loads in the reference (pix2pix.py:174-186)."""

    def save_global(self, obj, name=None):
        mod = getattr(obj, '__module__', None) or ''
        if mod.startswith('numpy._core'):
            nm = name or getattr(obj, '__qualname__', obj.__name__)
            self.write(pickle.GLOBAL + ('numpy.core' + mod[len('numpy._core'):]).encode() + b'\n' +
                       nm.encode() + b'\n')
            self.memoize(obj)
            return
        pickle._Pickler.save_global(self, obj, name)


class Pix2Pix:
    def _print_network(self, l_out):
        for layer in L.get_all_layers(l_out):
            print(layer, layer.output_shape, "" if not hasattr(layer, 'nonlinearity') else layer.nonlinearity)
        print("# learnable params:", L.count_params(l_out, trainable=True))

    def __init__(self,
                 gen_fn_dcgan, disc_fn_dcgan,
                 gen_params_dcgan, disc_params_dcgan,
                 gen_fn_p2p, disc_fn_p2p,
                 gen_params_p2p, disc_params_p2p,
                 in_shp, latent_dim, is_a_grayscale, is_b_grayscale,
                 alpha=100, opt=adam, opt_args=None,
                 train_mode='both', reconstruction='l1', sampler=np.random.rand, lsgan=False, verbose=True,
                 device=None, comm=None, use_graph=True, seed=None, two_streams=True, force_exchange=False,
                 side_streams=None, dtype='bf16x3', bucket_mb=None, prefetch=True, exchange_mode=None, ema=None):
        """Two-stage DCGAN / pix2pix GAN (see the reference docstring, pix2pix.py:32-64).
        gen_fn_dcgan(latent_dim, is_a_grayscale, **gen_params_dcgan) -> output layer
        disc_fn_dcgan(in_shp, is_a_grayscale, **disc_params_dcgan) -> output layer
        gen_fn_p2p(in_shp, is_a_grayscale, is_b_grayscale, **gen_params_p2p) -> output layer
        disc_fn_p2p(in_shp, is_a_grayscale, is_b_grayscale, **disc_params_p2p) -> {"inputs": [a, b], "out": layer}
        opt / opt_args: a lasagne.updates rule of gan_heightmaps_amd.updates -- sgd, momentum, nesterov_momentum, adagrad,
        rmsprop, adadelta, adam, adamax or amsgrad -- and its kwargs; 'learning_rate' may be a shared scalar, the
        other hyper-parameters are numbers (default adam with shared(1e-3), pix2pix.py:30).
        ema: a decay in [0, 1), e.g. 0.999 -- keep an exponential moving average of the two generators' parameters on the
        device, behind every update, and use it through ``ema_weights()`` / ``save_model(ema=True)`` (not in the
        reference).  None (default): no average, nothing changes."""
        assert train_mode in ['dcgan', 'p2p', 'both']
        assert reconstruction in ['l1', 'l2']
        if opt_args is None:
            opt_args = {'learning_rate': shared(floatX(1e-3))}
        self.is_a_grayscale = is_a_grayscale
        self.is_b_grayscale = is_b_grayscale
        self.latent_dim = latent_dim
        self.sampler = sampler
        self.in_shp = in_shp
        self.verbose = verbose
        self.train_mode = train_mode
        # train(): with host-array iterators the batch of step i+1 is drawn and uploaded (copy stream + page-locked staging)
        # while step i runs (GanStep.train_pipelined); False keeps the reference's strictly sequential upload -> step -> read
        self.prefetch = bool(prefetch)
        if seed is not None:
            _init.set_rng(np.random.RandomState(seed))
        # construction order fixes the RNG draw order of the initial weights (pix2pix.py:73-77)
        dcgan_gen = gen_fn_dcgan(latent_dim, is_a_grayscale, **gen_params_dcgan)
        dcgan_disc = disc_fn_dcgan(in_shp, is_a_grayscale, **disc_params_dcgan)
        p2p_gen = gen_fn_p2p(in_shp, is_a_grayscale, is_b_grayscale, **gen_params_p2p)
        p2p_disc = disc_fn_p2p(in_shp, is_a_grayscale, is_b_grayscale, **disc_params_p2p)
        if verbose:
            for label, net in [("dcgan gen:", dcgan_gen), ("dcgan disc:", dcgan_disc), ("p2p gen:", p2p_gen),
                               ("p2p disc:", p2p_disc["out"])]:
                print(label)
                self._print_network(net)
            print("train_mode: %s" % train_mode)
        self.dcgan = {'gen': dcgan_gen, 'disc': dcgan_disc}
        self.p2p = {'gen': p2p_gen, 'disc': p2p_disc["out"]}
        spec = opt(**opt_args)
        if not isinstance(spec, OptimizerSpec) or spec.kind not in OPT_RULES:
            raise TypeError("opt must be one of gan_heightmaps_amd.updates.{%s}" % ", ".join(OPT_RULES))
        self.lr = opt_args['learning_rate'] if 'learning_rate' in opt_args else spec.learning_rate
        if device is None:
            # one process per GPU: the launcher's LOCAL_RANK names this process' device (a communicator brings its own)
            device = Device(comm.dev.index) if comm is not None else Device(int(os.environ.get("LOCAL_RANK", "0")))
        self.device = device
        self.comm = comm
        self.engine = GanStep(self.device, dcgan_gen, dcgan_disc, p2p_gen, p2p_disc, alpha, lsgan, reconstruction,
                              spec, train_mode, comm=comm, use_graph=use_graph, two_streams=two_streams,
                              force_exchange=force_exchange, side_streams=side_streams, dtype=dtype,
                              bucket_mb=bucket_mb, exchange_mode=exchange_mode, ema=ema)
        self.train_keys = list(TRAIN_KEYS)
        eng = self.engine
        eng.broadcast_parameters()          # replicas start from rank 0's (possibly unseeded) initial weights
        if ema is not None:
            eng.reset_ema()                 # the averages start from the weights every replica now holds
        self.train_fn = lambda Z, X, Y: eng.train(floatX(Z), floatX(X), floatX(Y))
        self._engine_train_fn = self.train_fn      # train() pipelines uploads only while train_fn is still the engine's own
        self.loss_fn = lambda Z, X, Y: eng.loss(floatX(Z), floatX(X), floatX(Y))
        self.gen_fn = lambda X: eng.generate('p2p_gen', X, False)
        self.gen_fn_det = lambda X: eng.generate('p2p_gen', X, True)
        self.z_fn = lambda Z: eng.generate('dcgan_gen', Z, False)
        self.z_fn_det = lambda Z: eng.generate('dcgan_gen', Z, True)

    def texture_heightmap(self, heightmap, overlap=None, batch_size=4, out=None, uint8=False, deterministic=True):
        """Texture a heightmap of any size: overlapping in_shp x in_shp tiles through gen_fn_det's forward plan, the overlaps
        cross-faded (gan_heightmaps_amd/texture.py).  Not in the reference.
        heightmap: (H, W) or (H, W, C_a) uint8 (normalised as the training path does), or (C_a, H, W) float32 already
        normalised; any array that slices by rows (np.memmap, an HDF5 dataset) works.  overlap: tile overlap in pixels,
        0 .. in_shp / 2 (default in_shp / 4).  Returns (C_out, H, W) float32, or with uint8=True the (H, W, 3) uint8 RGB
        of util.to_uint8(util.convert_to_rgb(.)); ``out`` (that shape and dtype) is written in place of a new array.
        Leaves the training state untouched."""
        from .texture import texture_heightmap
        return texture_heightmap(self.engine, heightmap, self.is_a_grayscale, self.is_b_grayscale, overlap=overlap,
                                 batch_size=batch_size, out=out, uint8=uint8, deterministic=deterministic)

    def generate_terrain(self, grid=None, z=None, blend='bilinear', band=None, out=None, uint8=False, deterministic=True):
        """One seamless heightmap of gy x gx generator outputs from a grid of latent vectors: the DCGAN generator's head
        runs per cell, the cells' seed maps form one canvas ('mosaic', or 'bilinear' blending between neighbouring cells),
        and the fully convolutional trunk runs over the canvas in row windows with an exact halo
        (gan_heightmaps_amd/terrain.py).  Not in the reference.
        grid=(gy, gx) draws z from ``self.sampler`` (numpy's global RNG, like generate_gz); or give z [gy, gx, latent_dim].
        band: seed rows kept per window (default: a fixed memory budget).  Returns (C_a, in_shp gy, in_shp gx) float32, or
        with uint8=True util.to_uint8(util.convert_to_rgb(.)) as (H, W) for a greyscale generator, (H, W, 3) otherwise;
        ``out`` (that shape and dtype, e.g. an open_memmap) is written in place of a new array.  Leaves the training state
        untouched."""
        from .terrain import generate_terrain
        return generate_terrain(self.engine, self.dcgan['gen'], self.latent_dim, self.sampler, self.is_a_grayscale,
                                grid=grid, z=z, blend=blend, band=band, out=out, uint8=uint8, deterministic=deterministic)

    def terrain_world(self, seed, **kw):
        """An unbounded terrain of this model addressed by pixel coordinates: a TerrainWorld whose ``heightmap`` /
        ``texture`` / ``both`` (y0, x0, h, w) return any rectangle of the world of ``seed``, negative coordinates included.
        A pixel is a pure function of (weights, seed, coordinates): requests made at different times, in any order, agree
        bit for bit where they overlap.  The world is cut into chunks of ``chunk_cells`` generator outputs a side, each from
        one trunk pass over a world-anchored seed window with an exact halo; chunks are cached in HBM (``cache_mb``) and
        recomputed after the parameters change; textures are world-anchored U-Net tiles gathered on the device
        (gan_heightmaps_amd/world.py).  Not in the reference.
        kw: chunk_cells (default: a fixed memory budget; part of the world's identity), blend ('bilinear' | 'mosaic'),
        overlap (texture tiles, default in_shp / 4), batch_size (tiles per pass), cache_mb, latent_fn(i, j) -> [latent_dim]
        in place of the seeded sampler draw, erosion (an erosion.Erosion: the world is then the eroded one, every chunk
        eroded over a window with an exact halo).  Use it as a context manager, or close() it.  Leaves the
        training state untouched."""
        from .world import TerrainWorld
        return TerrainWorld(self, seed, **kw)

    def erode_heightmap(self, heightmap, erosion=None, **kw):
        """Erode a heightmap with a pipe-model water simulation on the GPU (gan_heightmaps_amd/erosion.py).  Not
        in the reference.  heightmap: (H, W) or (1, H, W), floating point in [0, 1] (what a greyscale generator returns) or
        uint8; the array's edge is a wall.  erosion: an erosion.Erosion (default Erosion()); kw: erode's (fused, water,
        out, uint8).  Returns the eroded heightmap in the input's shape, float32 in [0, 1].  Leaves the training state
        untouched."""
        from .erosion import erode
        from .step import LANE_OF
        self.engine.sync()
        return erode(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, erosion, **kw)

    def sky_visibility(self, heightmap, sky=None, **kw):
        """The light of the sky on a heightmap, a horizon scan baked on the GPU (gan_heightmaps_amd/skylight.py, DESIGN
        §4r).  Not in the reference.  heightmap: (H, W), floating point in [0, 1] or uint8; sky: a skylight.SkyLight (default
        SkyLight()); kw: bake's (height_scale, margin, out, uint8, tiled).  Returns the (H, W) plane, float32 in [0, 1]: 1
        where the whole sky is seen.  Leaves the training state untouched."""
        from .skylight import bake
        from .step import LANE_OF
        self.engine.sync()
        return bake(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, sky, **kw)

    def heightmap_mesh(self, heightmap, max_error, tile=None, fused=None):
        """A heightmap as an adaptive triangle mesh, cut on the GPU (gan_heightmaps_amd/mesh.py).  Not in the
        reference.  heightmap: (H, W) or (1, H, W), floating point in [0, 1] or uint8, of any size (edge-replicated to whole
        tiles); max_error: the tolerance in height units; tile: the root square side, a power of two (None: the largest
        <= 256 that does not exceed the shorter side); fused: mesh.ErrorMap's.  Returns a mesh.TerrainMesh (``save`` writes
        .glb / .obj / .npz).  Leaves the training state untouched."""
        from .mesh import heightmap_mesh
        from .step import LANE_OF
        self.engine.sync()
        return heightmap_mesh(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, max_error, tile=tile, fused=fused)

    def heightmap_hydrology(self, heightmap, **kw):
        """Where the water is on a heightmap: filled lakes, flow directions, drainage area and basins, computed on the GPU
        (gan_heightmaps_amd/hydrology.py).  Not in the reference.  heightmap: (H, W) or (1, H, W), floating point
        (what a greyscale generator returns) or uint8; the array's edge is the outlet.  kw: analyse's (tiled, keep).
        Returns a hydrology.Hydrology with the planes ``filled``, ``depth``, ``direction``, ``accumulation`` and ``basin``.
        Leaves the training state untouched."""
        from .hydrology import analyse
        from .step import LANE_OF
        self.engine.sync()
        return analyse(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, **kw)

    def paint_water(self, texture, hydro, water=None):
        """The lakes and rivers of ``hydro`` (heightmap_hydrology's) painted on a texture of the same size.  Not
        in the reference.  texture: as this model's generators or the uint8 paths return it; water: a hydrology.Water
        (default Water()).  Returns the painted texture in the form it came in; dry pixels are untouched.  Intended use:

            hydro = model.heightmap_hydrology(heightmap)
            painted = model.paint_water(texture, hydro)
            Scene(hydro.filled, painted)                                            # renders lakes as flat blue surfaces
            model.heightmap_mesh(hydro.filled, 0.01).save(path, texture=painted)    # exports them

        Leaves the training state untouched."""
        from .hydrology import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, hydro, water, value_range=self.is_b_grayscale)

    def heightmap_routes(self, heightmap, sources, **kw):
        """How to get from anywhere on a heightmap to the nearest of ``sources`` ((row, col) cells: towns), and where the roads
        would run: the least-cost travel field, computed on the GPU (gan_heightmaps_amd/route.py).  Not in the
        reference.  heightmap: (H, W) or (1, H, W), floating point or uint8.  kw: route.field's (travel, hydro, penalty, tiled,
        keep).  Returns a route.CostField with the planes ``cost``, ``parent``, ``territory`` and ``traffic`` and the methods
        ``travel_cost(cell)`` and ``path(cell)``.  Intended use:

            hydro = model.heightmap_hydrology(heightmap)
            roads = model.heightmap_routes(hydro.filled, towns, hydro=hydro)      # lakes and rivers cost extra
            painted = model.paint_roads(model.paint_water(texture, hydro), roads, roads.paths(villages))

        Leaves the training state untouched."""
        from .route import field
        from .step import LANE_OF
        self.engine.sync()
        return field(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, sources, **kw)

    def paint_roads(self, texture, cost_field, paths=(), road=None):
        """Roads painted on a texture of the field's size.  Not in the reference.  cost_field: heightmap_routes';
        paths: what its ``path`` / ``paths`` return; with ``road.traffic_threshold`` the cells that at least so many cells travel
        through are painted instead.  road: a route.Road (default Road()).  Returns the painted texture in the form it came in;
        other pixels are untouched.  Leaves the training state untouched."""
        from .route import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, cost_field, paths, road, value_range=self.is_b_grayscale)

    def carve_heightmap(self, heightmap, marks, target, profile, **kw):
        """A heightmap shaped towards ``target`` around the marked cells, on the GPU (gan_heightmaps_amd/earthworks.py, DESIGN
        §4v).  Not in the reference.  marks: an integer plane, marked where >= ``threshold``; target: a float plane read at the
        marked cells alone; profile: an earthworks.Profile; kw: earthworks.carve's (threshold, tiled, keep, origin).  Returns an
        earthworks.Earthworks with ``height`` and the volumes ``cut`` and ``fill``.  Leaves the training state untouched."""
        from .earthworks import carve
        from .step import LANE_OF
        self.engine.sync()
        return carve(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, marks, target, profile, **kw)

    def cut_rivers(self, hydro, channel=None, **kw):
        """River channels cut into the filled surface of ``hydro`` (heightmap_hydrology's).  Not in the reference.
        channel: an earthworks.Channel (default Channel()); kw: earthworks.carve's (tiled, keep, origin).  Returns an
        earthworks.Earthworks.  Intended use:

            hydro = model.heightmap_hydrology(heightmap)
            roads = model.heightmap_routes(hydro.filled, towns, hydro=hydro)
            ground = model.cut_rivers(hydro).height
            ground = model.grade_roads(ground, roads, roads.paths(villages)).height      # what Scene and heightmap_mesh take

        Leaves the training state untouched."""
        from .earthworks import cut_rivers
        from .step import LANE_OF
        self.engine.sync()
        return cut_rivers(self.engine.ops[LANE_OF['dcgan_gen']], hydro, channel, **kw)

    def grade_roads(self, heightmap, cost_field, paths=(), roadbed=None, traffic_threshold=None, **kw):
        """Roadbeds graded into a heightmap of the field's size.  Not in the reference.  cost_field:
        heightmap_routes'; paths: what its ``path`` / ``paths`` return; with ``traffic_threshold`` the cells that at least so
        many cells travel through are graded instead.  roadbed: an earthworks.Roadbed (default Roadbed()); kw:
        earthworks.carve's (tiled, keep, origin).  Returns an earthworks.Earthworks.  Leaves the training state untouched."""
        from .earthworks import grade_roads
        from .step import LANE_OF
        self.engine.sync()
        return grade_roads(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, cost_field, paths, roadbed, traffic_threshold, **kw)

    def scatter_heightmap(self, heightmap, species, **kw):
        """Trees and rocks placed on a heightmap by Poisson-disk sampling, on the GPU (gan_heightmaps_amd/scatter.py, DESIGN
        §4w).  Not in the reference.  species: a scatter.Species or a list of them; kw: scatter.scatter's (seed, origin, hydro,
        roads, blocked, height_scale, tiled, keep).  Returns a scatter.Scatter: per species the points, their heights, yaws
        and scales.  Intended use:

            hydro = model.heightmap_hydrology(heightmap)
            forest = model.scatter_heightmap(hydro.filled, [scatter.Species("rock", 9.0), scatter.Species("pine", 4.0,
                                             seed_stream=1)], hydro=hydro)            # the wider spacing first
            painted = model.paint_scatter(texture, forest, [(0.5, 0.5, 0.5), (0.1, 0.3, 0.1)])
            model.heightmap_mesh(hydro.filled, max_error).save("land.glb", texture=painted, instances=forest)

        Leaves the training state untouched."""
        from .scatter import scatter
        from .step import LANE_OF
        self.engine.sync()
        return scatter(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, species, **kw)

    def paint_scatter(self, texture, scatter, colours=(0.10, 0.28, 0.12), radius=1, opacity=0.9):
        """A texture (this model's generators' or the uint8 paths', of the scatter's size) with the points of a scatter.Scatter
        painted on it, layer after layer, by the hydrology's paint kernel.  Not in the reference.  colours: three
        numbers in [0, 1] or one such triple per species; radius: pixels around a point, 0 .. 4.  Unpainted pixels keep their
        bits.  Leaves the training state untouched."""
        from .scatter import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, scatter, colours, radius, opacity,
                     value_range=self.is_b_grayscale)

    def heightmap_viewshed(self, heightmap, observers, sight=None, accel=None):
        """What a set of observers can see of a heightmap, by exact lines of sight on the GPU (gan_heightmaps_amd/viewshed.py,
        DESIGN §4x).  Not in the reference.  observers: (row, col), (row, col, eye_height) or (row, col, eye_height, max_dist)
        each; sight: a viewshed.Sight (default Sight()); accel: the form, the same bits either way.  Returns a
        viewshed.Viewshed with ``count`` and ``mask``.  Intended use:

            seen = model.heightmap_viewshed(heightmap, towers)
            roads = model.heightmap_routes(heightmap, towns, penalty=seen.count.astype(np.float32))      # roads out of sight
            forest = model.scatter_heightmap(heightmap, species, blocked=seen.visible(0))                # a clearing to look over
            painted = model.paint_viewshed(texture, seen, hidden=True)

        Leaves the training state untouched."""
        from .viewshed import viewshed
        from .step import LANE_OF
        self.engine.sync()
        return viewshed(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, observers, sight, accel)

    def paint_viewshed(self, texture, viewshed, colour=(1.0, 0.85, 0.2), opacity=0.5, hidden=False):
        """A texture (this model's generators' or the uint8 paths', of the viewshed's size) with the ground the observers of a
        viewshed.Viewshed see -- hidden=True: the ground none of them sees -- blended towards ``colour`` by the hydrology's
        paint kernel.  Not in the reference.  Unpainted pixels keep their bits.  Leaves the training state
        untouched."""
        from .viewshed import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, viewshed, colour, opacity, hidden,
                     value_range=self.is_b_grayscale)

    def heightmap_contours(self, heightmap, levels=None, **kw):
        """The contour lines of a heightmap as ordered polylines, traced on the GPU (gan_heightmaps_amd/contour.py).
        Not in the reference.  levels: a contour.Levels (default Levels(): a line every 4 cells of height, every fifth an index
        contour; count=1 is a single isoline at ``base``, a coastline); kw: contour.contours' (origin, max_segments, keep).
        Returns a contour.Contours.  Intended use:

            lines = model.heightmap_contours(heightmap)
            lines.save("sheet.svg", texture=texture)                                  # or .geojson, .npz
            coast = model.heightmap_contours(heightmap, Levels(base=sea_level, count=1))
            painted = model.paint_contours(texture, heightmap)

        Leaves the training state untouched."""
        from .contour import contours
        from .step import LANE_OF
        self.engine.sync()
        return contours(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, levels, **kw)

    def paint_contours(self, texture, heightmap, levels=None, colour=(0.25, 0.15, 0.05), opacity=0.6, index_opacity=0.9):
        """A texture (this model's generators' or the uint8 paths', of the heightmap's size) with the heightmap's contour lines
        drawn on it, a pixel wide, the index contours heavier, by the hydrology's paint kernel.  heightmap: the
        heightmap, or a contour.Contours that kept its 'zq'.  Not in the reference.  Unpainted pixels keep their bits.  Leaves
        the training state untouched."""
        from .contour import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, heightmap, levels, colour, opacity, index_opacity,
                     value_range=self.is_b_grayscale)

    def heightmap_peaks(self, heightmap, prominence=None, form=None, **kw):
        """The peaks of a heightmap -- summits with their prominence, key col and parent -- found on the GPU
        (gan_heightmaps_amd/peaks.py).  Not in the reference.  prominence: a peaks.Prominence (default Prominence():
        at least 8 cells above the key col); form: 'plain' or 'list', the same bits; kw: peaks.peaks' (origin, max_summits,
        keep).  Returns a peaks.Peaks.  Intended use:

            found = model.heightmap_peaks(heightmap, Prominence(top=10))
            seen = model.heightmap_viewshed(heightmap, found.observers(eye_height=10))
            lines.save("sheet.svg", peaks=found)                                      # the sheet's spot heights
            painted = model.paint_peaks(texture, found)

        Leaves the training state untouched."""
        from .peaks import peaks
        from .step import LANE_OF
        self.engine.sync()
        return peaks(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, prominence, form=form, **kw)

    def paint_peaks(self, texture, peaks, colour=(0.9, 0.1, 0.1), radius=2, cols=False):
        """A texture (this model's generators' or the uint8 paths', of the peaks' plane's size) with a dot of ``radius`` pixels on
        every peak of a peaks.Peaks -- cols: on every key col -- by the hydrology's paint kernel.  Not in the
        reference.  Unpainted pixels keep their bits.  Leaves the training state untouched."""
        from .peaks import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, peaks, colour, radius, cols, value_range=self.is_b_grayscale)

    def heightmap_rivers(self, heightmap_or_hydrology, network=None, form=None, **kw):
        """The rivers of a heightmap -- the stream network as ordered reaches with their Strahler orders, Shreve magnitudes and
        main stems -- traced on the GPU (gan_heightmaps_amd/rivers.py).  Not in the reference.
        heightmap_or_hydrology: a heightmap as ``heightmap_hydrology`` takes it, which is analysed first, or a
        hydrology.Hydrology that kept 'direction' and 'accumulation'; network: a rivers.Network (default Network(): a stream
        from 256 cells of drainage area on); form: 'plain' or 'list', the same bits; kw: rivers.rivers' (origin, max_reaches,
        keep).  Returns a rivers.Rivers.  Intended use:

            found = model.heightmap_rivers(heightmap, Network(min_order=2))
            lines.save("sheet.svg", peaks=tops, rivers=found)                         # the sheet's blue lines
            roads = model.heightmap_routes(heightmap, found.confluences())            # towns where rivers meet
            painted = model.paint_rivers(texture, found)

        Leaves the training state untouched."""
        from .hydrology import Hydrology, analyse
        from .rivers import rivers
        from .step import LANE_OF
        self.engine.sync()
        ops = self.engine.ops[LANE_OF['dcgan_gen']]
        hydro = heightmap_or_hydrology
        if not isinstance(hydro, Hydrology):
            hydro = analyse(ops, hydro, keep=('filled', 'depth', 'direction', 'accumulation'))
        return rivers(ops, hydro, network, form=form, **kw)

    def paint_rivers(self, texture, rivers, min_order=1, width=0, colour=None, opacity=0.85):
        """A texture (this model's generators' or the uint8 paths', of the rivers' plane's size) with the reaches of a
        rivers.Rivers of at least ``min_order`` drawn ``width`` pixels (0 .. 4) to either side by the hydrology's paint kernel
        (DESIGN §4za); colour: default the water's.  Not in the reference.  Unpainted pixels keep their bits.  Leaves the
        training state untouched."""
        from .hydrology import Water
        from .rivers import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, rivers, min_order, width, Water().colour if colour is None else colour,
                     opacity, value_range=self.is_b_grayscale)

    def heightmap_regions(self, labels_or_heightmap, of='lakes', areas=None, form=None, **kw):
        """The areas of a heightmap or of a label plane as polygons with holes -- an outer ring and its islands, in order, with
        the number of cells -- labelled and traced on the GPU (gan_heightmaps_amd/regions.py).  Not in the reference.
        labels_or_heightmap: an integer plane (H, W) is a label plane (negative: no region) and ``of`` is not read; a heightmap
        as ``heightmap_hydrology`` takes it is turned into one first: of='lakes' or 'basins' through its hydrology, 'land'
        (kw sea_level, a number in [0, 1]) or 'bands' (kw levels, a contour.Levels).  areas: a regions.Areas; form: 'sweep' or
        'union', the same bits; kw besides: regions.regions' (origin, keep, max_edges).  Returns a regions.Regions.  Intended use:

            water = model.heightmap_regions(heightmap, 'lakes', Areas(min_cells=16))
            water.save("lakes.geojson")
            lines.save("sheet.svg", regions=water)                                    # the sheet's filled lakes
            painted = model.paint_regions(texture, water, (0.2, 0.4, 0.8), 0.6)

        Leaves the training state untouched."""
        from . import regions as _rg
        from .hydrology import analyse
        from .step import LANE_OF
        self.engine.sync()
        ops = self.engine.ops[LANE_OF['dcgan_gen']]
        x = labels_or_heightmap
        if hasattr(x, "dtype") and np.asarray(x).ndim == 2 and np.asarray(x).dtype.kind in "iu" and np.asarray(x).dtype != np.uint8:
            labels = x
        elif of == 'lakes':
            labels = _rg.lakes(analyse(ops, x, keep=('depth',)), **({"lake_min_depth": kw.pop("lake_min_depth")} if "lake_min_depth" in kw else {}))
        elif of == 'basins':
            labels = _rg.basins(analyse(ops, x, keep=('basin',)))
        elif of == 'land':
            if "sea_level" not in kw:
                raise ValueError("of='land' needs sea_level")
            labels = _rg.land(x, kw.pop("sea_level"))
        elif of == 'bands':
            labels = _rg.bands(x, kw.pop("levels", None))
        else:
            raise ValueError("of must be 'lakes', 'basins', 'land' or 'bands', got %r" % (of,))
        return _rg.regions(ops, labels, areas, form=form, **kw)

    def paint_regions(self, texture, regions, colour=None, opacity=0.6, outline=False):
        """A texture (this model's generators' or the uint8 paths', of the regions' plane's size) with the polygons of a
        regions.Regions filled -- outline=True: their cells along the rings only -- by the hydrology's paint kernel (DESIGN
        §4zb); colour: default the water's.  Not in the reference.  Unpainted pixels keep their bits.  Leaves the training state
        untouched."""
        from .hydrology import Water
        from .regions import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, regions, Water().colour if colour is None else colour, opacity,
                     outline, value_range=self.is_b_grayscale)

    def heightmap_climate(self, heightmap, weather=None, biomes=None, hydrology=False, form=None, **kw):
        """The climate of a heightmap -- rain carried along the wind with its rain shadow, temperature from altitude and world
        row, a biome per cell and, with hydrology, the rain-weighted discharge -- computed on the GPU
        (gan_heightmaps_amd/climate.py).  Not in the reference.  heightmap: (H, W) or (1, H, W), uint8 or floats in
        [0, 1]; weather: a climate.Weather; biomes: a climate.Biomes; hydrology: True analyses the drainage first, or a
        hydrology.Hydrology that kept 'direction'; form: 'line' or 'staged', the same bits; kw: climate.analyse's (origin,
        keep).  Returns a climate.Climate.  Intended use:

            hydro = model.heightmap_hydrology(heightmap)
            c = model.heightmap_climate(heightmap, Weather(wind='SW'), hydrology=hydro)
            found = model.heightmap_rivers(c.hydrology(hydro))                        # rivers that are thin on the dry side
            zones = model.heightmap_regions(regions.biomes(c), of='labels')           # biome polygons
            trees = model.scatter_heightmap(heightmap, species, blocked=~c.mask('taiga', 'temperate forest'))
            painted = model.paint_biomes(texture, c, 0.5)

        Leaves the training state untouched."""
        from .climate import analyse
        from .hydrology import Hydrology, analyse as drainage
        from .step import LANE_OF
        self.engine.sync()
        ops = self.engine.ops[LANE_OF['dcgan_gen']]
        hydro = hydrology if isinstance(hydrology, Hydrology) else (drainage(ops, heightmap, keep=('direction',)) if hydrology else None)
        return analyse(ops, heightmap, weather, biomes, hydro=hydro, form=form, **kw)

    def paint_biomes(self, texture, climate, opacity=0.6):
        """A texture (this model's generators' or the uint8 paths', of the climate's plane's size) with every pixel blended
        towards its biome's colour in the chart by the climate's palette kernel.  Not in the reference.  The
        pixels of a biome without a colour keep their bits.  Leaves the training state untouched."""
        from .climate import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, climate, opacity, value_range=self.is_b_grayscale)

    def heightmap_sunlight(self, heightmap, sun=None, form=None, **kw):
        """Where the sun shines on a heightmap -- per cell the sun positions that light it, their hours and the energy on its
        slope -- by exact shadow rays on the GPU (gan_heightmaps_amd/sunlight.py).  Not in the reference.
        heightmap: (H, W) or (1, H, W), uint8 or floats in [0, 1]; sun: a sunlight.Sun (default sunlight.Day().sun(), an equinox
        day at 45 degrees north); form: 'plain' or 'accel', the same bits; kw: sunlight.sunlight's (origin, keep).  Returns a
        sunlight.Sunlight.  Intended use:

            light = model.heightmap_sunlight(heightmap, Day(latitude=47, declination=-23.44).sun())
            vines = model.scatter_heightmap(heightmap, species, blocked=~light.mask_hours(6))
            painted = model.paint_sunlight(texture, light, max_hours=2)

        Leaves the training state untouched."""
        from .sunlight import sunlight
        from .step import LANE_OF
        self.engine.sync()
        return sunlight(self.engine.ops[LANE_OF['dcgan_gen']], heightmap, sun, form, **kw)

    def paint_sunlight(self, texture, sunlight, max_hours, colour=(0.05, 0.05, 0.2), opacity=0.5):
        """A texture (this model's generators' or the uint8 paths', of the sunlight's size) with the cells a sunlight.Sunlight
        finds lit fewer than ``max_hours`` hours blended towards ``colour`` by the hydrology's paint kernel.  Not
        in the reference.  Unpainted pixels keep their bits.  Leaves the training state untouched."""
        from .sunlight import paint
        from .step import LANE_OF
        self.engine.sync()
        return paint(self.engine.ops[LANE_OF['dcgan_gen']], texture, sunlight, max_hours, colour, opacity,
                     value_range=self.is_b_grayscale)

    def render_terrain(self, heightmap, texture, camera, height_scale=None, sky=None, **kw):
        """A camera view of a heightmap and its texture (arrays as this model's generators or the uint8 paths return them),
        ray cast on the GPU (gan_heightmaps_amd/render.py).  Not in the reference.  camera: a render.Camera in
        the heightmap's pixel coordinates; sky: a skylight.SkyLight, the scene is lit from the sky; kw:
        Scene.render's (sun, shadows, haze, step, max_dist, uint8, out, accel).
        For many frames of one terrain build a render.Scene once instead.  Leaves the training state untouched."""
        from .render import DEFAULTS, Scene
        self.engine.sync()
        with Scene(heightmap, texture, height_scale=DEFAULTS['height_scale'] if height_scale is None else height_scale,
                   value_range=(self.is_a_grayscale, self.is_b_grayscale), device=self.device, sky=sky) as scene:
            return scene.render(camera, **kw)

    # ---- sliced Wasserstein distance of the generators (gan_heightmaps_amd/swd.py) ------------------------
    def _own_draw(self, rs, n):
        """``self.sampler``'s distribution drawn from the RandomState ``rs``: the samplers of numpy's global RNG (np.random.rand,
        randn, ...) are methods of a RandomState, and ``rs`` has the same method"""
        owner, name = getattr(self.sampler, '__self__', None), getattr(self.sampler, '__name__', None)
        if not isinstance(owner, np.random.RandomState) or not hasattr(rs, name or ''):
            raise ValueError("swd draws z from a RandomState of its own, which needs a sampler that is a method of numpy's "
                             "global RNG (np.random.rand, np.random.randn, ...); with %r pass z=[num_images, latent_dim]"
                             % (self.sampler,))
        return floatX(getattr(rs, name)(n, self.latent_dim))

    def _swd_real(self, iterator, num_images, batch_size, which, metric):
        """the real sets' descriptors (set 0) from ``num_images // batch_size`` batches of ``iterator`` -> a dict that
        _swd_fake compares generated sets with, any number of times; _swd_close frees it.  For 'p2p' the A batches are kept
        on the host: U(A) is computed from them at every comparison."""
        from .step import LANE_OF
        from .swd import SWD, Descriptors
        if which not in ('both', 'dcgan', 'p2p'):
            raise ValueError("which must be 'both', 'dcgan' or 'p2p', got %r" % (which,))
        metric = SWD() if metric is None else metric
        nb = int(num_images) // int(batch_size)
        if nb < 1:
            raise ValueError("num_images=%r gives no batch of %r" % (num_images, batch_size))
        n, eng, S = nb * batch_size, self.engine, self.in_shp
        ca, cb = (1 if self.is_a_grayscale else 3), (1 if self.is_b_grayscale else 3)
        st = {'n': n, 'batch_size': batch_size, 'metric': metric, 'nets': [k for k in ('dcgan', 'p2p') if which in ('both', k)],
              'A': [], 'real': {}}
        eng.sync()
        try:
            if 'dcgan' in st['nets']:
                st['real']['dcgan'] = Descriptors(eng.ops[LANE_OF['dcgan_gen']], metric, 0, n, ca, S, S, max_batch=batch_size)
            if 'p2p' in st['nets']:
                st['real']['p2p'] = Descriptors(eng.ops[LANE_OF['p2p_gen']], metric, 0, n, cb, S, S, max_batch=batch_size)
            for _ in range(nb):
                X, Y = self._next(iterator)
                X, Y = floatX(X), floatX(Y)
                if X.shape[0] != batch_size:
                    raise ValueError("the iterator returned a batch of %d images, not %d (a ragged last batch: choose a "
                                     "batch size that divides the dataset)" % (X.shape[0], batch_size))
                if 'dcgan' in st['real']:
                    st['real']['dcgan'].add(X)
                if 'p2p' in st['real']:
                    st['real']['p2p'].add(Y)
                    st['A'].append(X)
        except BaseException:
            self._swd_close(st)
            raise
        return st

    def _swd_fake(self, st, seed=0, z=None):
        """the distance of the current generators' sets (set 1) from the real ones of ``st``"""
        from .step import LANE_OF
        from .swd import Descriptors, distance
        eng, n, bs, S, metric = self.engine, st['n'], st['batch_size'], self.in_shp, st['metric']
        out = {}
        for net in st['nets']:
            key = net + '_gen'
            real = st['real'][net]
            if net == 'dcgan':
                zs = self._own_draw(np.random.RandomState(seed), n) if z is None else floatX(z)
                if zs.shape != (n, self.latent_dim):
                    raise ValueError("z must be [%d, %d], got %s" % (n, self.latent_dim, zs.shape))
            with Descriptors(eng.ops[LANE_OF[key]], metric, 1, n, real.C, S, S, max_batch=bs) as fake:
                for b in range(n // bs):
                    inp = zs[b * bs:(b + 1) * bs] if net == 'dcgan' else st['A'][b]
                    fake.add(eng.generate_device(key, inp, True))          # read from plan.out where it lies
                out[net] = distance(eng.ops[LANE_OF[key]], real, fake)
        return out

    @staticmethod
    def _swd_close(st):
        for d in st['real'].values():
            d.close()
        st['real'], st['A'] = {}, []

    def swd(self, iterator, num_images=1024, batch_size=4, which='both', metric=None, seed=0, z=None):
        """Sliced Wasserstein distance on Laplacian-pyramid patches between real and generated images, on the GPU
        (gan_heightmaps_amd/swd.py).  Not in the reference.  'dcgan' compares the iterator's A images with G(z),
        'p2p' its B images with U(A); ``which`` picks one or 'both'.  Returns {'dcgan': r, 'p2p': r} (or the one asked for),
        r = {'levels': [512, 256, ...], 'swd': [per level], 'mean': float}; smaller is closer.
        The iterator is advanced by ``num_images // batch_size`` batches and by nothing else; that many batches of
        ``batch_size`` images form each set.  z is drawn from a RandomState(seed) of the call's own with ``self.sampler``'s
        distribution (or given: [num_images, latent_dim]), never from ``self.sampler`` or numpy's global RNG.  metric: a
        swd.SWD (default SWD()).  The forwards are the deterministic ones (z_fn_det, gen_fn_det) and their outputs are read
        from device memory; the call works inside ``with model.ema_weights():`` and leaves the training state untouched."""
        st = self._swd_real(iterator, num_images, batch_size, which, metric)
        try:
            return self._swd_fake(st, seed, z)
        finally:
            self._swd_close(st)

    def ema_weights(self):
        """``with model.ema_weights(): ...`` -- inside the block both generators run on the exponential moving average of
        their parameters (Pix2Pix(ema=decay)): z_fn_det, gen_fn_det, generate_gz / generate_atob / the interpolations with
        deterministic=True, texture_heightmap, generate_terrain, terrain_world, get_all_param_values and save_model all see
        the averaged weights; BatchNorm running statistics stay the live ones.  The weights are exchanged with the average
        on the device on entry and exchanged back on exit (also when the body raises); ``param_version`` moves both times,
        so an open terrain_world recomputes its chunks.  Training, loss_fn, the non-deterministic forwards and every loader
        raise RuntimeError inside the block.  ValueError on a model without an average."""
        return self.engine.ema_weights()

    def reset_ema(self):
        """start the average again from the current weights (e.g. after a warm-up)"""
        self.engine.reset_ema()

    def _is_writer(self):
        """files (results.txt, PNG dumps, checkpoints) are written by rank 0 only; every rank still runs the
        forward passes and iterator draws of the per-epoch dumps, which are part of the training trajectory"""
        comm = getattr(self, 'comm', None)
        return comm is None or comm.rank == 0

    # ---- checkpoint (pix2pix.py:158-186): gzip + pickle of get_all_param_values per net -------------------
    def _model_dict(self, ema=False):
        eng = getattr(self, 'engine', None)
        gen = {'dcgan': 'dcgan_gen', 'p2p': 'p2p_gen'}
        values = (lambda st: eng.ema_values(gen[st])) if ema else (lambda st: L.get_all_param_values(getattr(self, st)['gen']))
        dd = {'dcgan': {'gen': values('dcgan'),
                        'disc': L.get_all_param_values(self.dcgan['disc'])},
              'p2p': {'gen': values('p2p'),
                      'disc': L.get_all_param_values(self.p2p['disc'])}}
        ls = eng.loss_scale_state() if hasattr(eng, 'loss_scale_state') else []
        if ls:          # fp16 only: the dynamic loss scale is training state (an extra key; the reference's loader ignores it)
            dd['loss_scale'] = [{k: float(v) for k, v in st.items()} for st in ls]
        return dd

    def save_model(self, filename, ema=False):
        """``ema=True``: the generators' averaged weights in place of the live ones (Pix2Pix(ema=decay)) -- a plain model file
        that load_model, the reference and every command-line tool read as they are"""
        if ema and getattr(getattr(self, 'engine', None), 'ema', None) is None:
            raise ValueError("save_model(ema=True): this model keeps no average (construct it with ema=<decay>)")
        if not self._is_writer():
            return
        dd = self._model_dict(ema)
        with gzip.open(filename, "wb") as g:
            _Py2CompatPickler(g, 2).dump(dd)      # protocol 2 == py2 HIGHEST_PROTOCOL, readable by the reference

    @staticmethod
    def _read_checkpoint(filename):
        with gzip.open(filename) as g:
            return pickle.load(g, encoding='latin1')      # genuine py2 checkpoints need latin1

    def _set_params(self, dd, mode):
        eng = getattr(self, 'engine', None)
        averaged = getattr(eng, 'ema', None) is not None
        if averaged:
            eng._live_only("loading parameters")
        if mode in ('both', 'dcgan'):
            L.set_all_param_values(self.dcgan['gen'], dd['dcgan']['gen'])
            L.set_all_param_values(self.dcgan['disc'], dd['dcgan']['disc'])
        if mode in ('both', 'p2p'):
            L.set_all_param_values(self.p2p['gen'], dd['p2p']['gen'])
            L.set_all_param_values(self.p2p['disc'], dd['p2p']['disc'])
        if dd.get('loss_scale') and mode == 'both':
            self.engine.restore_loss_scale_state(dd['loss_scale'])
        if averaged:        # the average of every generator just loaded restarts from the loaded weights
            eng.reset_ema([k for k, m in (('dcgan_gen', 'dcgan'), ('p2p_gen', 'p2p')) if mode in ('both', m)])

    def load_model(self, filename, mode='both'):
        assert mode in ['both', 'dcgan', 'p2p']
        self._set_params(self._read_checkpoint(filename), mode)

    # ---- full training state: the save_model file + one 'train_state' key ---------------------------------------------
    # save_model / load_model carry the parameters (and the fp16 loss scale) only; a run resumed from them restarts the
    # optimiser state, Adam's step counter, the dropout counters and the batch order.  A state checkpoint carries all of
    # it, so that resuming on the same world size, dtype, exchange mode and batch size continues bit for bit.
    TRAIN_STATE_VERSION = 1
    # gzip level of a state checkpoint.  Protocol 2 writes an array's bytes as latin-1 text (1.5x the fp32 size), which level 1
    # takes back to within 1 % of level 9's file at a fraction of its time; the fp32 values themselves hardly compress
    # (full-size Adam state on the MI355X's host: DESIGN §4h)
    checkpoint_compresslevel = 1

    def save_checkpoint(self, filename, iterators=None, epoch=None):
        """save_model's file plus the training state: the engine's (optimiser slots, [lr, t], dropout counters, loss-scale
        records), the learning rate, numpy's global RNG (the default sampler), ``{name: it.get_state()}`` of the
        ``iterators`` that have it, and ``epoch``.  Every rank calls it (the sharded update gathers its optimiser state);
        rank 0 writes, after checking that every rank's iterator and sampler RNG state is its own."""
        eng = self.engine
        ts = {'version': self.TRAIN_STATE_VERSION,
              'engine': eng.training_state(),
              'lr': self.lr.get_value() if hasattr(self.lr, 'get_value') else self.lr,
              'np_random': np.random.get_state(),
              'iterators': {name: it.get_state() for name, it in (iterators or {}).items() if hasattr(it, 'get_state')},
              'epoch': epoch}
        comm = getattr(self, 'comm', None)
        if comm is not None and comm.world > 1:
            import zlib
            from .step import crc_range
            lo, hi = crc_range(comm, zlib.crc32(pickle.dumps((ts['np_random'], ts['iterators']), 2)))
            if lo != hi:
                raise RuntimeError("save_checkpoint: the iterator / sampler RNG state differs between the ranks (every rank "
                                   "must draw the global batch and keep its slice); such a checkpoint cannot be resumed")
        if not self._is_writer():
            return
        dd = self._model_dict()
        dd['train_state'] = ts
        with gzip.open(filename, "wb", compresslevel=self.checkpoint_compresslevel) as g:
            _Py2CompatPickler(g, 2).dump(dd)

    def load_checkpoint(self, filename, iterators=None):
        """inverse of save_checkpoint: parameters, training state, learning rate, numpy's global RNG and the state of each
        of ``iterators`` (a dict name -> iterator, as given to save_checkpoint).  Returns the saved epoch."""
        return self._restore_checkpoint(self._read_checkpoint(filename), iterators)

    def _restore_checkpoint(self, dd, iterators):
        import warnings
        if getattr(getattr(self, 'engine', None), '_in_ema', False):
            self.engine._live_only("load_checkpoint")
        ts = dd.get('train_state')
        if ts is None:
            raise ValueError("no training state in this checkpoint (a save_model file: use load_model)")
        if ts.get('version') != self.TRAIN_STATE_VERSION:
            raise ValueError("training state format %r; this version reads %d" % (ts.get('version'), self.TRAIN_STATE_VERSION))
        self.engine.check_training_state(ts['engine'])         # before anything is changed
        self._set_params(dd, 'both')
        self.engine.restore_training_state(ts['engine'])
        if hasattr(self.lr, 'set_value'):
            self.lr.set_value(ts['lr'])         # (the engine's listener puts it into hyper[0])
        else:
            self.lr = ts['lr']
        np.random.set_state(ts['np_random'])
        for name, it in (iterators or {}).items():
            if hasattr(it, 'set_state') and name in ts['iterators']:
                it.set_state(ts['iterators'][name])
            else:
                warnings.warn("iterator %r: no saved state restored; its batch order will not be reproduced" % name,
                              RuntimeWarning)
        ls = ts['engine'].get('loss_scale')
        if ls:
            self._ls_prev = [st['skipped_steps'] for st in ls]
        return ts['epoch']

    # ---- training loop (pix2pix.py:187-275) ----------------------------------------------------------------
    def train(self, it_train, it_val, batch_size, num_epochs, out_dir, model_dir=None, save_every=10, resume=False,
              quick_run=False, validate_on_train_iterator=True, dump_images=True, checkpoint_state=False, swd_every=None,
              swd_iterator=None, swd_images=1024):
        """Same loop as the reference: per epoch N//batch_size train_fn steps then N//batch_size loss_fn steps,
        a CSV row of epoch means, then the per-epoch image dumps (a 4x4 grid of [A | U(A)] from ``it_val``, one batch of
        A->B pairs from each iterator, 20 DCGAN samples -- pix2pix.py:262-270; they advance the iterators, so they
        are part of the training trajectory; ``dump_images=False`` skips them), periodic checkpoints.  The
        reference's validation loop draws its batches from ``it_train`` (pix2pix.py:204);
        ``validate_on_train_iterator=True`` keeps that behaviour.  Checked event for event against the reference's
        own loop in tests/test_reference_trainloop.py.
        ``checkpoint_state=True``: the periodic checkpoints are save_checkpoint files (the whole training state, with both
        iterators'); ``resume`` may name either kind -- a state checkpoint continues the run, epoch numbers included, a
        save_model file loads the parameters only.
        ``swd_every=K``: every K epochs ``out_dir/swd.txt`` gets one row per trained generator -- epoch, 'live', net, the sliced
        Wasserstein distance per level, their mean (Pix2Pix.swd) -- and with ``ema`` a second row, 'ema', of the
        averaged weights.  The real sets' descriptors are computed once, before the first epoch, from ``swd_images`` images of
        ``swd_iterator``: an iterator of its own, since drawing from ``it_train`` / ``it_val`` would change the training
        trajectory (ValueError).  results.txt, the iterators' and the sampler's draws are what they are without it."""
        if getattr(getattr(self, 'engine', None), '_in_ema', False):
            self.engine._live_only("train")
        if swd_every is not None:
            if isinstance(swd_every, bool) or not isinstance(swd_every, (int, np.integer)) or swd_every < 1:
                raise ValueError("swd_every must be None or an integer >= 1, got %r" % (swd_every,))
            if swd_iterator is None or swd_iterator is it_train or swd_iterator is it_val:
                raise ValueError("swd_every needs swd_iterator, an iterator of its own: drawing the real sets from it_train "
                                 "or it_val would change the training trajectory")

        def _next(it):
            return next(it) if hasattr(it, '__next__') else it.next()

        def _loop(fn, itr, src):
            rec = [[] for _ in self.train_keys]
            on_device = hasattr(src, 'next_into')          # gan_heightmaps_amd.data.Hdf5Iterator: batch stays in HBM
            eng = getattr(self, 'engine', None)
            own = fn is getattr(self, 'train_fn', None) and fn is getattr(self, '_engine_train_fn', None)   # (a replaced / wrapped train_fn is called as it is)
            if (own and not on_device and getattr(self, 'prefetch', False)
                    and hasattr(eng, 'train_pipelined')):
                # host arrays: the same draws in the same order, but batch i+1 is drawn, sampled and uploaded (copy stream,
                # page-locked staging) while step i runs; losses bit-identical to the call-by-call form
                def batches():
                    for _ in range(itr.N // batch_size):
                        X_batch, Y_batch = _next(src)
                        yield floatX(self.sampler(X_batch.shape[0], self.latent_dim)), floatX(X_batch), floatX(Y_batch)
                        if quick_run:
                            break
                try:
                    for results in eng.train_pipelined(batches()):
                        for i, r in enumerate(results):
                            rec[i].append(r)
                except BaseException:
                    eng.close_pipeline()        # an abandoned loop must not leave an upload in flight on the copy stream
                    raise
                return tuple(np.mean(elem) for elem in rec)
            if (own and on_device and getattr(self, 'prefetch', False)
                    and hasattr(eng, 'train_pipelined_from_iterator')):
                steps = 1 if quick_run else itr.N // batch_size
                try:
                    for results in eng.train_pipelined_from_iterator(src, lambda n: floatX(self.sampler(n, self.latent_dim)), steps):
                        for i, r in enumerate(results):
                            rec[i].append(r)
                except BaseException:
                    eng.close_pipeline()
                    raise
                return tuple(np.mean(elem) for elem in rec)
            for _ in range(itr.N // batch_size):
                if on_device:
                    results = self.engine.run_from_iterator(
                        src, lambda n: floatX(self.sampler(n, self.latent_dim)), train=fn is self.train_fn)
                else:
                    X_batch, Y_batch = _next(src)
                    Z_batch = floatX(self.sampler(X_batch.shape[0], self.latent_dim))
                    results = fn(Z_batch, X_batch, Y_batch)
                for i, r in enumerate(results):
                    rec[i].append(r)
                if quick_run:
                    break
            return tuple(np.mean(elem) for elem in rec)

        header = ["epoch"] + ["train_%s" % k for k in self.train_keys] + ["valid_%s" % k for k in self.train_keys] \
            + ["lr", "time", "mode"]
        writer = self._is_writer()
        if writer:
            os.makedirs(out_dir, exist_ok=True)
            if model_dir is not None:
                os.makedirs(model_dir, exist_ok=True)
        f = open("%s/results.txt" % out_dir if writer else os.devnull, "w" if not resume else "a")
        first = 0
        if not resume:
            f.write(",".join(header) + "\n")
            f.flush()
            if self.verbose:
                print(",".join(header))
        else:
            if self.verbose:
                print("loading weights from: %s" % resume)
            dd = self._read_checkpoint(resume)
            if 'train_state' in dd:
                first = self._restore_checkpoint(dd, {'train': it_train, 'valid': it_val}) or 0
            else:
                self._set_params(dd, 'both')
            del dd
        swd_st, swd_f = None, None
        if swd_every is not None:
            from . import swd as _swd
            swd_st = self._swd_real(swd_iterator, swd_images, batch_size, self.train_mode, None)
            levels = [min(hw) for hw in next(iter(swd_st['real'].values())).sizes]
            swd_f = open("%s/swd.txt" % out_dir if writer else os.devnull, "w" if not resume else "a")
            if not resume:
                swd_f.write(",".join(_swd.header(levels)) + "\n")
                swd_f.flush()
        for e in range(first, first + num_epochs):
            t0 = time()
            row = [str(e + 1)]
            row += [str(v) for v in _loop(self.train_fn, it_train, it_train)]
            row += [str(v) for v in _loop(self.loss_fn, it_val, it_train if validate_on_train_iterator else it_val)]
            lr = self.lr.get_value() if hasattr(self.lr, 'get_value') else self.lr
            row += [str(lr), str(time() - t0), self.train_mode]
            line = ",".join(row)
            if self.verbose:
                print(line)
            f.write(line + "\n")
            f.flush()
            self._check_loss_scale(e + 1)
            if swd_st is not None and (e + 1) % swd_every == 0:
                rows = [('live', self._swd_fake(swd_st))]
                if getattr(self.engine, 'ema', None) is not None:
                    with self.ema_weights():
                        rows.append(('ema', self._swd_fake(swd_st)))
                for weights, res in rows:
                    for net in swd_st['nets']:
                        swd_f.write(",".join(_swd.row(e + 1, weights, net, res[net])) + "\n")
                swd_f.flush()
            if dump_images:
                with util_writes(writer):
                    if self.train_mode in ['both', 'p2p']:
                        plot_grid("%s/out_%i.png" % (out_dir, e + 1), it_val, self.gen_fn,
                                  is_a_grayscale=self.is_a_grayscale, is_b_grayscale=self.is_b_grayscale)
                        self.generate_atob(it_train, 1, "%s/dump_train" % out_dir, deterministic=False)
                        self.generate_atob(it_val, 1, "%s/dump_valid" % out_dir, deterministic=False)
                    if self.train_mode in ['both', 'dcgan']:
                        self.generate_gz(num_examples=20, batch_size=batch_size, out_dir="%s/dump_a" % out_dir,
                                         deterministic=False)
            if model_dir is not None and (e + 1) % save_every == 0:
                if checkpoint_state:
                    self.save_checkpoint("%s/%i.model" % (model_dir, e + 1), {'train': it_train, 'valid': it_val}, e + 1)
                else:
                    self.save_model("%s/%i.model" % (model_dir, e + 1))
                if getattr(getattr(self, 'engine', None), 'ema', None) is not None:
                    self.save_model("%s/%i.ema.model" % (model_dir, e + 1), ema=True)
        f.close()
        if swd_st is not None:
            swd_f.close()
            self._swd_close(swd_st)

    def _check_loss_scale(self, epoch):
        """fp16 only: one line per epoch with the dynamic loss scale and the updates it skipped, and a warning when
        training has stalled on it -- a scale at its floor with every step still flagged means the FORWARD activations
        exceed the fp16 range, which no loss scale can fix (use bf16)"""
        eng = getattr(self, 'engine', None)
        ls = eng.loss_scale_state() if hasattr(eng, 'loss_scale_state') else []
        if not ls:
            return
        prev = getattr(self, '_ls_prev', [0] * len(ls))
        skipped = [st['skipped_steps'] - p for st, p in zip(ls, prev)]
        self._ls_prev = [st['skipped_steps'] for st in ls]
        if self.verbose:
            print("epoch %d: fp16 loss scale %s, updates skipped this epoch %s"
                  % (epoch, [st['scale'] for st in ls], skipped))
        for st, sk in zip(ls, skipped):
            if st['scale'] <= self.engine.ls_min and sk > 0:
                import warnings
                warnings.warn("fp16 loss scale is at its minimum (%g) and %d updates were skipped in epoch %d: the "
                              "activations overflow fp16; training is stalled -- use dtype='bf16'"
                              % (st['scale'], sk, epoch), RuntimeWarning)

    # ---- sampling helpers (pix2pix.py:276-425): forward-only, PNG output through util.imsave (PIL) --------
    @staticmethod
    def _next(itr):
        return next(itr) if hasattr(itr, '__next__') else itr.next()

    def generate_atob(self, itr, num_batches, out_dir, dont_predict=False, deterministic=True):
        """pix2pix samples (pix2pix.py:276-305): for every element of ``num_batches`` batches write
        ``<ctr>.a.png`` (the input A) and ``<ctr>.b.png`` (U(A), or the iterator's own B when
        ``dont_predict``)."""
        fn = self.gen_fn_det if deterministic else self.gen_fn
        makedirs(out_dir)
        ctr = 0
        for _ in range(num_batches):
            this_x, this_y = self._next(itr)
            pred_y = this_y if dont_predict else fn(this_x)
            for i in range(pred_y.shape[0]):
                imsave("%s/%i.a.png" % (out_dir, ctr), convert_to_rgb(this_x[i], is_grayscale=self.is_a_grayscale))
                imsave("%s/%i.b.png" % (out_dir, ctr), convert_to_rgb(pred_y[i], is_grayscale=self.is_b_grayscale))
                ctr += 1

    def generate_gz(self, num_examples, batch_size, out_dir, deterministic=True):
        """DCGAN samples g(z) (pix2pix.py:306-326): one draw of ``sampler(num_examples, latent_dim)``,
        ``num_examples // batch_size`` forward passes, ``<ctr>.png`` each."""
        makedirs(out_dir)
        fn = self.z_fn_det if deterministic else self.z_fn
        z = floatX(self.sampler(num_examples, self.latent_dim))
        ctr = 0
        for b in range(num_examples // batch_size):
            out = fn(z[b * batch_size:(b + 1) * batch_size])
            for i in range(out.shape[0]):
                imsave("%s/%i.png" % (out_dir, ctr), convert_to_rgb(out[i], is_grayscale=self.is_a_grayscale))
                ctr += 1

    def interpolation_grid(self, zsample1=None, zsample2=None, deterministic=True, mode='row'):
        """The decoded interpolation of generate_interpolation as an array [rows, cols, H, W, 3]:
        'row' = 1x6 with coefficients (0, .1, .3, .6, .9, 1), 'matrix' = 5x5 with linspace(0, 1, 25)
        (pix2pix.py:344-368).  All coefficients go through the generator as ONE batch (the reference
        runs 6 / 25 batch-1 calls; with deterministic BN the result per sample is the same)."""
        assert mode in ['row', 'matrix']
        fn = self.z_fn_det if deterministic else self.z_fn
        if zsample1 is None:
            zsample1 = floatX(self.sampler(1, self.latent_dim))[0]
        if zsample2 is None:
            zsample2 = floatX(self.sampler(1, self.latent_dim))[0]
        zsample1, zsample2 = np.asarray(zsample1), np.asarray(zsample2)
        if mode == 'row':
            rows, cols, coefs = 1, 6, np.asarray([0.0, 0.1, 0.3, 0.6, 0.9, 1.0], zsample1.dtype)
        else:
            rows, cols, coefs = 5, 5, np.linspace(0, 1, 25).astype(zsample1.dtype)
        z = (1 - coefs)[:, None] * zsample1[None] + coefs[:, None] * zsample2[None]
        if deterministic:
            out = fn(floatX(z))
        else:       # batch statistics would couple the samples: keep the reference's batch-1 calls
            out = np.concatenate([fn(floatX(z[i:i + 1])) for i in range(len(coefs))], axis=0)
        grid = np.zeros((rows, cols, self.in_shp, self.in_shp, 3), dtype=zsample1.dtype)
        for n in range(len(coefs)):
            grid[n // cols][n % cols] = convert_to_rgb(out[n], is_grayscale=self.is_a_grayscale)
        return grid

    def generate_interpolation(self, out_name, zsample1=None, zsample2=None, deterministic=True, mode='row',
                               figsize=(10, 10), cmap='gray'):
        """Write the interpolation grid between two prior samples as one figure (pix2pix.py:328-369)."""
        from . import image_grid
        grid = self.interpolation_grid(zsample1, zsample2, deterministic, mode)
        image_grid.write_image_grid(out_name, grid, figsize=figsize, cmap=cmap)

    def generate_interpolation_clip(self, num_samples, batch_size, out_dir, deterministic=True, min_max_norm=False,
                                    concat=False):
        """Frames of a long interpolation z1 -> z2 -> ... -> zn, 25 steps per leg, each decoded to a heightmap
        G(z) and textured by U(G(z)) (pix2pix.py:371-425).  The G -> U chain stays in HBM
        (GanStep.generate_chain); ``a_%04d.png``/``b_%04d.png`` or ``concat_%04d.png`` per frame."""
        os.makedirs(out_dir, exist_ok=True)
        zs = floatX(self.sampler(num_samples, self.latent_dim))
        coefs = np.linspace(0, 1, 25).astype(zs.dtype)
        legs = [(1 - coefs)[:, None] * zs[i][None] + coefs[:, None] * zs[i + 1][None] for i in range(len(zs) - 1)]
        all_z = np.concatenate(legs, axis=0).astype(zs.dtype) if legs else np.zeros((0, self.latent_dim), zs.dtype)
        ctr = 0
        for b in range(all_z.shape[0] // batch_size):
            z_out, p2p_out = self.engine.generate_chain(all_z[b * batch_size:(b + 1) * batch_size], deterministic)
            for i in range(z_out.shape[0]):
                a_img = z_out[i]
                if min_max_norm:
                    a_img = (a_img - np.min(a_img)) / (np.max(a_img) - np.min(a_img))
                a_img = convert_to_rgb(a_img, is_grayscale=self.is_a_grayscale)
                b_img = convert_to_rgb(p2p_out[i], is_grayscale=self.is_b_grayscale)
                d = '%04d' % ctr
                if concat:
                    imsave("%s/concat_%s.png" % (out_dir, d), np.concatenate([a_img, b_img], axis=1))
                else:
                    imsave("%s/a_%s.png" % (out_dir, d), a_img)
                    imsave("%s/b_%s.png" % (out_dir, d), b_img)
                ctr += 1
