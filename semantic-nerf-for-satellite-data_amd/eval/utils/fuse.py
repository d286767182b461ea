"""The median surface on the map: per-cell altitude quantiles over all views of a split, and the spread of the views' altitudes
-- the raster every multi-view stereo pipeline for satellites fuses its pairwise DSMs into, and a confidence raster that needs no
lidar.  The reference has no counterpart; the spec is include/snerf_fuse.h, the stages are the kernels of
csrc/fuse.hip, torch is plumbing.  All functions take and return device tensors.

The top surface (eval/utils/ortho.py) takes the highest point of any view in a cell and the mean DSM the mean of all of them: one
floater in one view owns the cell of the first and drags the second up by 1/m of its height, and where some views see a roof and
others the ground the mean lands in the air between them.  An order statistic has neither fault, but it cannot be folded with one
atomic per cell: it needs each cell's list.  So the clouds are walked twice --

  count_offers   every point adds 1 to the cells of its window (the lattice, the window and the validity rule of the top surface);
  offsets_of     the exclusive prefix sums of the counts cut ONE key buffer into a segment per cell (torch.cumsum on int64; the
                 one .item() for the total is the only host synchronisation before the results: select reads the stats back);
  scatter_keys   every offer stores the top surface's 64-bit key, (round((z - Z0)/Q) + 2^31) << 32 | (2^32 - 1 - global index),
                 in a slot of its cell's segment (an atomic cursor per cell hands out the slots);
  select         one wave per cell finds the keys of exact ranks ((m - 1) num) // den -- numpy's method="lower", so every word is
                 an actual point, whose altitude and index ortho.gather reads as it reads the top surface's words.

Everything is integer: the words are bit-reproducible and do not depend on image order, chunking or launch order.  The scatter
walk must see the clouds the count walk saw; where it does not, offers are counted (never written out of place), the cells they
belong to are zeroed and counted, and select raises."""
import ctypes as C

import torch

from ... import _lib
from . import dsm as D
from . import ortho as OR
from .dsm import grid_struct, new_stats

QUARTILES = ((1, 4), (1, 2), (3, 4))
MAX_QUANTILES = _lib.FUSE_MAX_QUANTILES


def _cloud(cloud):
    if not (torch.is_tensor(cloud) and cloud.is_cuda):
        raise ValueError("fuse: the cloud must be a GPU tensor (the HIP path has no CPU fallback)")
    return D.cloud_f64(cloud)


def count_offers(cloud, grid, radius=0, count=None, stats=None):
    """add the offers of `cloud` (N, 3) (east, north, alt) to the per-cell counts of `grid` -> (count (out_h, out_w) int32 holding
    the u32 words, stats); `count` / `stats`: accumulators of earlier calls (zeroed ones are made otherwise)"""
    g = grid_struct(grid)
    xyz = _cloud(cloud)
    if count is None:
        count = torch.zeros((g.out_h, g.out_w), dtype=torch.int32, device=xyz.device)
    if count.dtype != torch.int32 or count.numel() != D.cell_count(g, "a map"):
        raise ValueError(f"count must hold {g.out_h} x {g.out_w} int32 words")
    stats = new_stats(xyz.device) if stats is None else stats
    _lib.call("snerf_fuse_count", xyz, xyz.shape[0], g, radius, OR.Z0, OR.Q, count, stats, exc=ValueError)
    return count, stats


def offsets_of(count):
    """the segments of the key buffer: -> (offsets int64 (cells + 1), the exclusive prefix sums of the u32 counts; total, their sum,
    as a Python int -- the one host synchronisation of the feature)"""
    c = count.reshape(-1).to(torch.int64) & 0xFFFFFFFF
    offsets = torch.zeros(c.numel() + 1, dtype=torch.int64, device=count.device)
    torch.cumsum(c, 0, out=offsets[1:])
    return offsets, int(offsets[-1].item())


def scatter_keys(cloud, grid, offsets, cursor, keys, radius=0, index0=0, stats=None):
    """store the keys of `cloud`'s offers in their cells' segments of `keys` (int64 holding the u64 words; its length is the
    capacity) -> stats.  `offsets`: offsets_of's; `cursor` (cells) int32, zeroed before the first cloud and carried across the
    calls; `index0`: the global index of the cloud's first point, as for ortho.top_surface."""
    g = grid_struct(grid)
    xyz = _cloud(cloud)
    cells = D.cell_count(g, "a map")
    if offsets.dtype != torch.int64 or offsets.numel() != cells + 1:
        raise ValueError(f"offsets must hold {cells} + 1 int64 words")
    if cursor.dtype != torch.int32 or cursor.numel() != cells:
        raise ValueError(f"cursor must hold {cells} int32 words")
    if keys.dtype != torch.int64 or keys.dim() != 1 or not keys.numel():
        raise ValueError("keys must be a non-empty 1-D int64 tensor")
    stats = new_stats(xyz.device) if stats is None else stats
    _lib.call("snerf_fuse_scatter", xyz, xyz.shape[0], index0, g, radius, OR.Z0, OR.Q, offsets, keys.numel(), cursor, keys, stats,
              exc=ValueError)
    return stats


def quantile_table(quantiles):
    """((num, den), ...) -> the host table snerf_fuse_select takes (a ctypes int array) and K.  The entry's own checks are made
    here first: a ctypes int array takes an integer beyond 32 bits without a word, by cutting it"""
    qs = [(int(a), int(b)) for a, b in quantiles]
    if not 1 <= len(qs) <= MAX_QUANTILES:
        raise ValueError(f"fuse: {len(qs)} quantiles, between 1 and {MAX_QUANTILES} are taken at once")
    for num, den in qs:
        if not (1 <= den <= 65536 and 0 <= num <= den):
            raise ValueError(f"fuse: quantile ({num}, {den}): 0 <= num <= den and 1 <= den <= 65536 required")
    return (C.c_int * (2 * len(qs)))(*[v for pair in qs for v in pair]), len(qs)


def select(keys, offsets, cursor, quantiles, h, w, stats=None, words=None):
    """the words of exact rank ((m - 1) num) // den of every cell's segment -> words (K, h, w) int64 holding the u64 keys, 0 where
    a cell has no offer.  Raises ValueError naming the counts when offers were dropped (stats[2], the scatter walk's) or cells
    refused (stats[3]): the scatter walk did not see what the count walk saw.  `stats`: the block the walks wrote."""
    table, K = quantile_table(quantiles)
    cells = h * w
    if offsets.dtype != torch.int64 or offsets.numel() != cells + 1 or cursor.dtype != torch.int32 or cursor.numel() != cells:
        raise ValueError(f"select: offsets must hold {cells} + 1 int64 words and cursor {cells} int32 words")
    if words is None:
        words = torch.empty((K, h, w), dtype=torch.int64, device=keys.device)
    if words.dtype != torch.int64 or tuple(words.shape) != (K, h, w) or not words.is_contiguous():
        raise ValueError(f"select: words must be a contiguous int64 tensor of shape {(K, h, w)}")
    stats = new_stats(keys.device) if stats is None else stats
    _lib.call("snerf_fuse_select", keys, offsets, keys.numel(), cursor, cells, table, K, words, stats, exc=ValueError)
    dropped, refused = (int(v) for v in stats[2:4].cpu())
    if dropped or refused:
        raise ValueError(f"fuse.select: {dropped} offer(s) found no slot and {refused} cell(s) were refused: the scatter walk did not "
                         "see the clouds of the count walk")
    return words


def fuse_walks(walk, grid, radius=0, quantiles=QUARTILES):
    """The two walks and the select.  `walk()` gives an iterator of (cloud, index0) pairs and is called twice -- once to count, once
    to scatter --, so a caller that cannot hold every cloud at once makes them again (ortho_products); both calls must give the same
    clouds, or select raises.  -> (words (K, H, W) int64, offers (H, W) int32, stats)"""
    g = grid_struct(grid)
    count = stats = None
    for cloud, _ in walk():
        count, stats = count_offers(cloud, g, radius, count, stats)
    if count is None:
        raise ValueError("fuse: no cloud")
    offsets, total = offsets_of(count)
    keys = torch.empty(max(total, 1), dtype=torch.int64, device=count.device)      # (an empty tensor has no address to pass)
    cursor = torch.zeros(count.numel(), dtype=torch.int32, device=count.device)
    for cloud, index0 in walk():
        scatter_keys(cloud, g, offsets, cursor, keys, radius, index0, stats)
    return select(keys, offsets, cursor, quantiles, g.out_h, g.out_w, stats), count, stats


def fuse_clouds(clouds, grid, radius=0, quantiles=QUARTILES, index0s=None):
    """fuse_walks over `clouds` (a list of (N_i, 3) device clouds; index0s: their global first indices, default the running
    offset) -> {"words" (K, H, W) int64, "offers" (H, W) int32 (how many points offered themselves to a cell), "alt" (K, H, W) f32
    (NaN where empty), "index" (K, H, W) int64 (-1 where empty), "stats"}."""
    clouds = list(clouds)
    if index0s is None:
        index0s, at = [], 0
        for c in clouds:
            index0s.append(at)
            at += c.shape[0]
    words, count, stats = fuse_walks(lambda: zip(clouds, index0s), grid, radius, quantiles)
    return dict(planes(words), words=words, offers=count, stats=stats)


def planes(words):
    """the altitude and the global point index of every word, plane by plane through ortho.gather, unchanged:
    {"alt" (K, H, W) f32, "index" (K, H, W) int64}"""
    got = [OR.gather(w, 0, 1) for w in words]
    return {"alt": torch.stack([o["alt"] for o in got]), "index": torch.stack([o["index"] for o in got])}


def spread(words_lo, words_hi, q=OR.Q):
    """q (k_hi - k_lo) as f32, k the quantised altitudes of two planes of words: the integer difference is exact; NaN where a
    cell is empty (a word is 0)"""
    k_lo, k_hi = (words_lo >> 32) & 0xFFFFFFFF, (words_hi >> 32) & 0xFFFFFFFF      # the u64 words' high halves: k + 2^31
    out = ((k_hi - k_lo).to(torch.float64) * q).to(torch.float32)
    return torch.where((words_lo == 0) | (words_hi == 0), torch.full_like(out, float("nan")), out)
