"""The reference's figure callbacks (core/figures/types.py:42-359) on the HIP path: the same files, drawn from the same
host random draws, with the frames of a figure rendered in a few batched generator calls instead of one call per
frame.  Every figure is three stages:

    plan(module)           host: latents from ``module.noise_distn`` (torch's global generator) and views from
                           ``generator.sample_view`` (numpy's), in the reference's order and dtypes
    render(module, plan)   GPU: the cell images of every frame, in frame-then-cell order ([F * n, C, H, W]), and the
                           uint8 frames (functional.figure_frames_u8: make_grid + clamp + x * 255 truncated)
    write(frames, epoch)   host: the PNG (imageio's min / max stretch of an integer array, restated) or the GIF
                           (forward then backward, PIL with the reference's arguments)

``render_per_frame`` renders the same cells the way the reference does -- one generator call per frame (per column
for the step grids) -- and exists for the tests and tools/figures_bench.py.  When a figure is drawn (the ``monitor``
rule) is the runner's business (run_network.EpochFigures); the module is expected in eval mode under no_grad there.

HoloGAN's AzimuthStep / AzimuthGif deviate from the reference, whose versions call ``generator(z, cameras=...)`` with a
camera model HoloGAN does not have (``#TODO: make this work for hologan``, types.py:213) and fail: here they sweep the
azimuth over ``linspace(azimuth_low, azimuth_high, n)`` at the middle elevation, with views built like ElevationStep's.
"""
import math
import os

import numpy as np
import torch

from ..utils.utils import interpolate_sphere

GEN_ROWS = 256          # images per batched generator call


def _has_views(generator):
    return hasattr(generator, "render_views") and hasattr(generator, "sample_view")


def _noise(module, n):
    return module.noise_distn.sample((n, module.cfg.model.noise_dim))


def _generate(generator, z, views=None, rows=GEN_ROWS):
    """generator(z) / generator(z, view_in=views) over chunks of ``rows`` images (eval mode: every image depends on its
    own latent and view alone)."""
    dev = next(generator.parameters()).device
    out = []
    for i in range(0, z.shape[0], rows):
        zi = z[i:i + rows].to(dev)
        out.append(generator(zi) if views is None else generator(zi, view_in=views[i:i + rows]))
    return out[0] if len(out) == 1 else torch.cat(out)


def _sweep_views(low, high, n, fixed, sweep_azimuth):
    """[n, 6] float32 views, element for element as the reference builds them (types.py:199-200, 234-235,
    309-311): the swept angle ``i * pi / 180`` in fp32 tensor arithmetic on ``torch.linspace(low, high, n)``, the fixed
    one ``fixed * pi / 180`` in Python double, both stored as fp32."""
    swept = torch.linspace(low, high, n) * math.pi / 180
    rows = []
    for s in swept:
        pair = [s, fixed * math.pi / 180] if sweep_azimuth else [fixed * math.pi / 180, s]
        rows.append(torch.tensor(pair + [1.0, 0, 0, 0]))
    return torch.stack(rows)


def png_array(frame_u8):
    """What imageio 2.9's ``imwrite`` stores for the reference's ``(array * 255).astype(int)`` (an int64 array):
    ``image_as_uint`` stretches min..max to 0..255 -- ``(im - mi) / (ma - mi) * 255 + 0.499999999`` in float64, then
    uint8 -- and leaves a constant image as it is."""
    im = np.asarray(frame_u8).astype(np.int64)
    mi, ma = im.min(), im.max()
    if ma == mi:
        return im.astype(np.uint8)
    return ((im.astype(np.float64) - mi) / (ma - mi) * (np.power(2.0, 8) - 1) + 0.499999999).astype(np.uint8)


class Figure:
    """reference Figure (types.py:42-91): ``<parent_dir>/<cfg.dir>/[epoch_<e>/]<cfg.filename or ClassName.png>``."""
    ext = ".png"
    needs_views = False          # a 3-D figure: the generator must take views (HoloGAN)

    def __init__(self, cfg, parent_dir, monitor=None):
        self.save_dir = os.path.join(parent_dir, cfg.dir)
        self.filename = cfg.filename if cfg.filename else type(self).__name__ + self.ext
        os.makedirs(self.save_dir, exist_ok=True)
        self.monitor = monitor
        self.current_best_metric = np.inf
        self.save_all = cfg.save_all

    # -- when (reference on_validation_end, :78-91) ------------------------------------------------------------------
    def should_draw(self, score):
        """The monitor rule: with a monitor, only a strictly better ``score`` than the best so far (which it becomes);
        ``score`` None (no metric produced) or no monitor: always."""
        if self.monitor and score is not None:
            if score < self.current_best_metric:
                self.current_best_metric = score
                print("Drawing & saving %s..." % self.filename)
                return True
            print("Current metric %s is worse than current best %s. Skipping figures"
                  % (score, self.current_best_metric))
            return False
        print("Drawing & saving %s..." % self.filename)
        return True

    # -- the three stages --------------------------------------------------------------------------------------------
    def check_generator(self, generator):
        if self.needs_views and not _has_views(generator):
            raise ValueError("%s is a 3-D figure: the generator (%s) has no views to sweep" %
                             (type(self).__name__, type(generator).__name__))

    def plan(self, module):
        raise NotImplementedError

    def render(self, module, plan):
        """-> (cells [F * n, C, H, W] float, frames uint8 [F, GH, GW, 3]) on the module's device."""
        from ... import functional as F
        cells = self.render_cells(module, plan)
        return cells, F.figure_frames_u8(cells, plan["frames"], plan["ncol"])

    def render_per_frame(self, module, plan):
        """The same as render() the way the reference computes it: one generator call per frame / column and one
        grid per frame."""
        from ... import functional as F
        cells = self.render_cells_per_frame(module, plan)
        n = cells.shape[0] // plan["frames"]
        frames = [F.figure_frames_u8(cells[i * n:(i + 1) * n], 1, plan["ncol"]) for i in range(plan["frames"])]
        return cells, torch.cat(frames)

    def out_path(self, epoch):
        d = os.path.join(self.save_dir, "epoch_%d" % epoch) if self.save_all else self.save_dir
        return os.path.join(d, self.filename)

    def write(self, frames, epoch):
        """frames: uint8 [1, GH, GW, 3] (the reference's ``(array * 255).astype(int)`` values)."""
        from PIL import Image
        path = self.out_path(epoch)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(png_array(np.asarray(frames)[0])).save(path)
        return path

    def draw(self, module):
        """plan + render: the uint8 frames as a numpy array."""
        plan = self.plan(module)
        return self.render(module, plan)[1].cpu().numpy()

    def draw_and_save(self, module, epoch):
        return self.write(self.draw(module), epoch)


class AnimationFigure(Figure):
    """reference AnimationFigure (types.py:93-135): the frames forward then backward, one GIF."""
    ext = ".gif"

    def __init__(self, cfg, parent_dir, monitor=None, n_frames=40):
        super().__init__(cfg, parent_dir, monitor)
        self.n_frames = n_frames

    def write(self, frames, epoch):
        """frames: uint8 [F, GH, GW, 3]; written as the 2F frames ``frames + frames[::-1]`` with PIL's GIF writer and
        the reference's arguments (types.py:115-130)."""
        from PIL import Image
        path = self.out_path(epoch)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        arrays = list(np.asarray(frames))
        pil = [Image.fromarray(np.ascontiguousarray(a[:, :, :3]), "RGB") for a in arrays + arrays[::-1]]
        pil[0].save(path, save_all=True, append_images=pil[1:], optimize=False, duration=self.n_frames, loop=0)
        return path


# ---------------------------------------------------------------------------------------------------------------------
class SampleGrid(Figure):
    """ncol x ncol samples (types.py:169-180).  HoloGAN: the view of each sample is the one its forward would draw."""

    def __init__(self, cfg, parent_dir, monitor=None, ncol=4):
        super().__init__(cfg, parent_dir, monitor)
        self.ncol = ncol

    def plan(self, module):
        z = _noise(module, self.ncol ** 2)
        views = module.generator.sample_view(self.ncol ** 2) if _has_views(module.generator) else None
        return {"z": z, "views": views, "frames": 1, "ncol": self.ncol}

    def render_cells(self, module, plan):
        return _generate(module.generator, plan["z"], plan["views"])

    render_cells_per_frame = render_cells


class Interpolation(AnimationFigure):
    """Spherical interpolation between two sets of 16 latents, 4 x 4 per frame (types.py:241-264); all frames' images
    in a few batched calls.  A generator with views draws one view set per frame, as its forward would."""
    per_frame = 16
    ncol = 4

    def plan(self, module):
        z1, z2 = _noise(module, 16), _noise(module, 16)
        ts = np.linspace(0, 1, self.n_frames)
        views = [module.generator.sample_view(16) for _ in ts] if _has_views(module.generator) else None
        return {"z1": z1, "z2": z2, "ts": ts, "views": views, "frames": len(ts), "ncol": self.ncol}

    def latents(self, module, plan):
        dev = next(module.generator.parameters()).device
        z1, z2 = plan["z1"].to(dev), plan["z2"].to(dev)
        return [interpolate_sphere(z1, z2, float(t))[:self.per_frame] for t in plan["ts"]]

    def frame_views(self, plan):
        return plan["views"]

    def render_cells(self, module, plan):
        views = self.frame_views(plan)
        return _generate(module.generator, torch.cat(self.latents(module, plan)),
                         None if views is None else np.concatenate(views))

    def render_cells_per_frame(self, module, plan):
        views = self.frame_views(plan)
        return torch.cat([_generate(module.generator, z, None if views is None else views[i])
                          for i, z in enumerate(self.latents(module, plan))])


class Interpolation3d(Interpolation):
    """Latents AND views interpolated (types.py:266-293): ``p = p2 * t + p1 * (1 - t)`` in float64 per frame."""
    needs_views = True

    def plan(self, module):
        self.check_generator(module.generator)
        z1, z2 = _noise(module, 16), _noise(module, 16)
        p1, p2 = module.generator.sample_view(16), module.generator.sample_view(16)
        ts = np.linspace(0, 1, self.n_frames)
        return {"z1": z1, "z2": z2, "p1": p1, "p2": p2, "ts": ts, "frames": len(ts), "ncol": self.ncol}

    def frame_views(self, plan):
        return [plan["p2"] * t + plan["p1"] * (1 - t) for t in plan["ts"]]


class _ViewSweep:
    """Shared by the step grids and the view GIFs: ``n_objs`` objects under ``n_views`` views built by _sweep_views."""
    needs_views = True
    sweep_azimuth = False

    def sweep(self, module, n_objs, n_views):
        self.check_generator(module.generator)
        z = _noise(module, n_objs)
        a = module.cfg.generator.view_args
        if self.sweep_azimuth:
            views = _sweep_views(a.azimuth_low, a.azimuth_high, n_views, (a.elevation_high + a.elevation_low) / 2, True)
        else:
            views = _sweep_views(a.elevation_low, a.elevation_high, n_views, (a.azimuth_high + a.azimuth_low) / 2, False)
        return z, views

    def objects_by_views(self, module, plan):
        """[n_objs, n_views, C, H, W] through Generator.render_views (the 3-D trunk once per object)."""
        dev = next(module.generator.parameters()).device
        return module.generator.render_views(plan["z"].to(dev), plan["views"])

    def objects_by_views_per_frame(self, module, plan):
        """The reference's loop: one generator call per view, all objects under it."""
        n = plan["z"].shape[0]
        cols = [_generate(module.generator, plan["z"], v.repeat(n, 1)) for v in plan["views"]]
        return torch.stack(cols).permute(1, 0, 2, 3, 4)


class ElevationStep(_ViewSweep, Figure):
    """Rows = objects, columns = elevation steps at the middle azimuth (types.py:217-239)."""

    def __init__(self, cfg, parent_dir, monitor=None, n_steps=8, n_objs=4):
        super().__init__(cfg, parent_dir, monitor)
        self.n_steps, self.n_objs, self.ncol = n_steps, n_objs, n_steps

    def plan(self, module):
        z, views = self.sweep(module, self.n_objs, self.n_steps)
        return {"z": z, "views": views, "frames": 1, "ncol": self.ncol}

    def render_cells(self, module, plan):
        r = self.objects_by_views(module, plan)
        return r.reshape(-1, *r.shape[2:])

    def render_cells_per_frame(self, module, plan):
        r = self.objects_by_views_per_frame(module, plan)
        return r.reshape(-1, *r.shape[2:])


class AzimuthStep(ElevationStep):
    """Rows = objects, columns = azimuth steps at the middle elevation (deviation: see the module docstring)."""
    sweep_azimuth = True


class ElevationGif(_ViewSweep, AnimationFigure):
    """``num_objs`` objects (the first 16 shown, 4 x 4) per frame, one frame per elevation (types.py:295-322)."""
    ncol = 4

    def __init__(self, cfg, parent_dir, num_objs=16, monitor=None, n_frames=40):
        super().__init__(cfg, parent_dir, monitor, n_frames=n_frames)
        self.num_objs = num_objs

    def shown(self):
        return min(self.num_objs, 16)

    def plan(self, module):
        z, views = self.sweep(module, self.num_objs, self.n_frames)
        return {"z": z, "views": views, "frames": self.n_frames, "ncol": self.ncol}

    def render_cells(self, module, plan):
        plan = dict(plan, z=plan["z"][:self.shown()])          # objects that are not shown are not rendered
        r = self.objects_by_views(module, plan).transpose(0, 1).contiguous()       # [views, objects, ...]
        return r.reshape(-1, *r.shape[2:])

    def render_cells_per_frame(self, module, plan):
        r = self.objects_by_views_per_frame(module, plan)[:self.shown()].transpose(0, 1).contiguous()
        return r.reshape(-1, *r.shape[2:])


class AzimuthGif(ElevationGif):
    """ncol x ncol objects per frame, one frame per azimuth at the middle elevation (types.py:324-359; deviation: see
    the module docstring)."""
    sweep_azimuth = True

    def __init__(self, cfg, parent_dir, ncol=4, monitor=None, n_frames=40):
        super().__init__(cfg, parent_dir, num_objs=ncol ** 2, monitor=monitor, n_frames=n_frames)
        self.ncol = ncol

    def shown(self):
        return self.ncol ** 2


def build_figures(cfg, module, parent_dir):
    """One figure per ``cfg.figures`` entry in its order (reference run_network.py:42-46): ``cfg=figure_details``,
    ``parent_dir``, ``monitor='fid'`` when ``figure_details.fid_callback``.  A 3-D figure configured for a generator
    without views is refused here, before any training."""
    from ...config import instantiate
    details = cfg.figure_details
    figs = [instantiate(node, cfg=details, parent_dir=parent_dir, monitor="fid" if details.fid_callback else None)
            for node in (cfg.get("figures") or {}).values()]
    for f in figs:
        f.check_generator(module.generator)
    return figs
