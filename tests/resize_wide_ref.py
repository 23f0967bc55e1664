"""Inputs and fp64 references of the wide resize + argmax tests (lc2is_resize_argmax*_wide, 193 to 1024 classes), shared by
tests/test_resize_argmax_wide_cpu.py and tests/test_gpu_resize_argmax_wide.py.  The references are those of the narrow tests:
torch's fp64 bicubic + argmax with the top-2 margin (slide_ref.ref_argmax), slide_ref's canvas mean and multiscale_ref's
softmax-sum / sum with their near-tie rules; only the class counts and the seeds are new.

The near-tie cap (slide_ref.UNSURE_CAP per case and size) is a condition on the inputs.  With 45 pixels at (5, 9) one unsure pixel
is 2.2e-2, and at (33, 17) three are 5.3e-3, so a seed is usable only if the fp64 reference alone leaves no pixel inside the
margin at (5, 9) and (1, 1) and at most two at (33, 17).  SEEDS holds, per kernel and class count, the first seed from 0 for
which that holds at every size (and, for multiscale, in both modes); the CPU test asserts it, so a change to a generator or a
case that breaks it is seen without a GPU."""
import functools

import torch

import multiscale_ref as M
import slide_ref as R

KS = (193, 257, 847, 1024)     # the first class count past the narrow limit; ld = 260 with a one-channel last chunk and the ninth
                               # bit of pred; ADE20K-full; the limit
SIZES = ((50, 90), (37, 53), (5, 9), (33, 17), (1, 1))   # several tiles with partial edge tiles, twice; the downscale band path
GRID = (10, 12)                # score-grid cells of the single-grid case
PLANT = 6.0                    # added to class 256 at K = 257 on the left half of the grid: on random logits it wins nowhere

SLIDE_ARGS = R.FP64_CASES[0][0][1:]                      # the "small" slide case without its class count: 8-cell views, 8 x 14 canvas
SLIDE_SIZES = tuple(R.FP64_CASES[0][1])
MS_SPECS, MS_SIZES = M.CASES["small"][2], M.CASES["small"][3]
MS_H = M.CASES["small"][1]

# first usable seed from 0 (see the module docstring), found by tests/test_resize_argmax_wide_cpu.py's condition
SEEDS = {
    "grid": {193: 0, 257: 0, 847: 0, 1024: 0},
    "slide": {193: 0, 257: 1, 847: 0, 1024: 0},
    "ms": {193: 3, 257: 3, 847: 1, 1024: 1},
}


@functools.lru_cache(maxsize=None)
def grid_logits(K, seed=None):
    """[1, K, 10, 12] randn logits of the single-grid kernel; at K = 257 class 256 is raised on the left half."""
    g = torch.Generator().manual_seed(SEEDS["grid"][K] if seed is None else seed)
    x = torch.randn(1, K, *GRID, generator=g)
    if K == 257:
        x[:, 256, :, :GRID[1] // 2] += PLANT
    return x


@functools.lru_cache(maxsize=None)
def grid_reference(K, size, seed=None):
    """(argmax, sure mask, unsure share) of grid_logits(K) at one output size: tests/test_gpu_resize_argmax.py's rule."""
    x = grid_logits(K, seed)
    ref, margin = R.ref_argmax(x[0], size)
    sure = margin > R.MARGIN * x.abs().max().item()
    return ref, sure, (~sure).float().mean().item()


def slide_case(K, seed=None):
    """(views, windows) of the "small" slide case at K classes."""
    return R.make_case(K, *SLIDE_ARGS, seed=SEEDS["slide"][K] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def slide_reference(K, size, seed=None):
    views, windows = slide_case(K, seed)
    Hc, Wc = SLIDE_ARGS[1], SLIDE_ARGS[2]
    ref, margin = R.ref_argmax(R.canvas_mean(views, windows, Hc, Wc, torch.float64), size)
    sure = margin > R.MARGIN * views.abs().max().item()
    return ref, sure, (~sure).float().mean().item()


@functools.lru_cache(maxsize=None)
def ms_case(K, seed=None):
    """multiscale_ref.make_case("small") at K classes: (views, canvases of one image, max |value| on the canvases)."""
    g = torch.Generator().manual_seed(SEEDS["ms"][K] if seed is None else seed)
    views, canvases, amax, v0 = [], [], 0.0, 0
    for Hc, Wc, stride, flip in MS_SPECS:
        v, wl, m = M.make_canvas(K, MS_H, Hc, Wc, stride, flip, g, v0)
        views.append(v); canvases.append(((Hc, Wc), tuple(wl))); amax = max(amax, m); v0 += len(v)
    return torch.cat(views).contiguous(), tuple(canvases), amax


@functools.lru_cache(maxsize=None)
def ms_reference(K, size, mode, seed=None):
    views, canvases, amax = ms_case(K, seed)
    return M.ref_argmax(views, canvases, size, mode, amax)


def usable(unsure_by_size):
    """The condition a seed must meet: every size's unsure share at or under the cap."""
    return all(u <= R.UNSURE_CAP for u in unsure_by_size.values())


def recount(pred, gt, k, ignore_index=None):
    """{intersection, predicted, labelled} [3, k] on the host (tests/test_gpu_slide.py's).  ignore_index None: every pixel is
    predicted, labelled where 0 <= gt < k; an int: only pixels with 0 <= gt < k and gt != ignore_index count, in all three rows."""
    p, g = pred.reshape(-1).long().cpu(), gt.reshape(-1).long().cpu()
    lab = (g >= 0) & (g < k)
    if ignore_index is not None:
        lab &= g != ignore_index
    predicted = p if ignore_index is None else p[lab]
    return torch.stack([torch.bincount(p[lab & (p == g)], minlength=k), torch.bincount(predicted, minlength=k),
                        torch.bincount(g[lab], minlength=k)]).int()
