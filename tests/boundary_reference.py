"""numpy restatement of the sl_boundary_counts contract (include/segland_hip.h), the per-class erosion form of the published Boundary IoU, and the label
maps the boundary tests share.

contract_counts is a brute-force statement of the contract: every map is padded with OUT and compared with each of its (2d+1)^2 shifted copies.  It knows nothing of
the kernel's separable, bit-parallel form.  erosion_counts follows Cheng et al.'s mask_to_boundary per class (zero border, d erosions with a 3x3 element, boundary =
mask - eroded) and is defined for maps without ignored pixels only."""
import numpy as np

IGN, OUT = 255, 254            # any two bytes above the 64 classes; the kernel's own codes differ and do not matter


def effective_labels(pred, target, K, ignore_index):
    """(T, P) uint8 [B,H,W] of the contract: T = target where it is a class and not ignore_index, else IGN; P = IGN where T is IGN or pred >= K, else pred."""
    pred, target = np.asarray(pred), np.asarray(target)
    T = np.where((target >= 0) & (target < K) & (target != ignore_index), target, IGN).astype(np.uint8)
    P = np.where((T == IGN) | (pred >= K), IGN, pred).astype(np.uint8)
    return T, P


def band(L, d):
    """band_L of one image [H,W]: some label of the (2d+1)^2 square differs from the centre; outside the image lies OUT."""
    H, W = L.shape
    pad = np.full((H + 2 * d, W + 2 * d), OUT, np.uint8)
    pad[d:d + H, d:d + W] = L
    b = np.zeros((H, W), bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            b |= pad[dy:dy + H, dx:dx + W] != L
    return b


def contract_counts(pred, target, K, ignore_index, d):
    """(counts [3][K], band_cm [K][K], share of the pixels in band_T, share in band_P), int64 counts, over a batch [B,H,W]."""
    T, P = effective_labels(pred, target, K, ignore_index)
    counts, cm = np.zeros((3, K), np.int64), np.zeros((K, K), np.int64)
    ng = npb = 0
    for b in range(T.shape[0]):
        gb, pb = band(T[b], d), band(P[b], d)
        ng, npb = ng + int(gb.sum()), npb + int(pb.sum())
        for k in range(K):
            g, p = (T[b] == k) & gb, (P[b] == k) & pb
            counts[0, k] += (g & p).sum()
            counts[1, k] += g.sum()
            counts[2, k] += p.sum()
        m = gb & (T[b] != IGN) & (P[b] != IGN)
        np.add.at(cm, (T[b][m].astype(np.int64), P[b][m].astype(np.int64)), 1)
    return counts, cm, ng / T.size, npb / T.size


def erode(mask, d):
    """d erosions of a boolean [H,W] mask with the 3x3 element, zeros beyond the border."""
    try:
        from scipy import ndimage
        return ndimage.binary_erosion(mask, np.ones((3, 3), bool), iterations=d, border_value=0)
    except ImportError:
        H, W = mask.shape
        for _ in range(d):
            pad = np.zeros((H + 2, W + 2), bool)
            pad[1:-1, 1:-1] = mask
            mask = np.ones((H, W), bool)
            for dy in range(3):
                for dx in range(3):
                    mask &= pad[dy:dy + H, dx:dx + W]
        return mask


def erosion_counts(pred, target, K, d):
    """counts [3][K] the published way: per class, boundary = mask & ~eroded for the ground truth and the prediction (every pixel a class: no ignore)."""
    pred, target = np.asarray(pred), np.asarray(target)
    assert target.min() >= 0 and target.max() < K and pred.max() < K
    counts = np.zeros((3, K), np.int64)
    for b in range(target.shape[0]):
        for k in range(K):
            g, p = target[b] == k, pred[b] == k
            gb, pb = g & ~erode(g, d), p & ~erode(p, d)
            counts[0, k] += (gb & pb).sum()
            counts[1, k] += gb.sum()
            counts[2, k] += pb.sum()
    return counts


def confusion(pred, target, K, ignore_index):
    """The whole-image confusion matrix of sl_confusion_matrix."""
    T, P = effective_labels(pred, target, K, ignore_index)
    m = (T != IGN) & (P != IGN)
    cm = np.zeros((K, K), np.int64)
    np.add.at(cm, (T[m].astype(np.int64), P[m].astype(np.int64)), 1)
    return cm


# ---------------------------------------------------------------------------------------------------------------------------------------------------- label maps
def seeds_of(H, W, n, rng, spread):
    """n seed points (float y, x).  spread 1: anywhere on the map.  spread < 1: the first in the centre, the others in the bottom-right corner of that share of each
    side, so that one cell is large enough to hold pixels whose whole (2d+1)^2 square is one label even where d is a large part of the map."""
    if spread >= 1.0:
        return np.stack([rng.uniform(0, H, n), rng.uniform(0, W, n)], 1)
    s = np.stack([rng.uniform((1 - spread) * H, H, n), rng.uniform((1 - spread) * W, W, n)], 1)
    s[0] = (0.5 * H, 0.5 * W)
    return s


def seed_classes(n, K):
    """A class per seed: the highest and the lowest class first, then distinct ones while K has them."""
    c = [(K - 1 - i * max(1, (K - 1) // max(1, n - 1))) % K for i in range(n)]
    if n > 1:
        c[1] = 0
    return np.asarray(c, np.int64)


def voronoi(H, W, seeds, classes):
    """[H,W] int64: every pixel takes the class of its nearest seed (the first one on a tie)."""
    y, x = np.mgrid[0:H, 0:W]
    dist = (y[None] - seeds[:, 0, None, None]) ** 2 + (x[None] - seeds[:, 1, None, None]) ** 2
    return classes[dist.argmin(0)]


# (B, H, W, K, d), seed spread, saturating (the whole map is band: exempt from the cover condition), with ignore / out-of-range pixels
CASES = {
    'ragged': ((2, 70, 131, 5, 3), 1.0, False, False),         # ragged tiles, batch-halo isolation
    'small': ((1, 16, 16, 3, 5), 0.07, False, False),          # map smaller than the tile
    'flat': ((1, 9, 200, 2, 32), 1.0, True, False),            # H < d: the whole map is band
    'row129': ((2, 129, 64, 33, 1), 1.0, False, False),        # smallest d; one row past the tile
    'lds': ((1, 160, 96, 64, 32), 0.07, False, False),         # largest K and d together: the LDS budget
    'ignore': ((3, 64, 64, 7, 4), 1.0, False, True),           # ignore rectangle, out-of-range targets, pred >= K
}
IGNORE_INDEX = 255
N_SEEDS = 6
PRED_SHIFT = (1.0, 2.0)        # the prediction's seeds: the target's, moved by this


def case_maps(name):
    """(pred uint8 [B,H,W], target int64 [B,H,W]) of a case, from a generator seeded by the case's name: the same arrays on every call."""
    (B, H, W, K, d), spread, _, dirty = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    pred, target = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.int64)
    for b in range(B):
        seeds, classes = seeds_of(H, W, N_SEEDS, rng, spread), seed_classes(N_SEEDS, K)
        target[b] = voronoi(H, W, seeds, classes)
        pred[b] = voronoi(H, W, seeds + np.asarray(PRED_SHIFT), classes).astype(np.uint8)
    if dirty:
        target[0, 10:30, 20:50] = IGNORE_INDEX                      # a rectangular ignore region
        target[2, :, 60:] = IGNORE_INDEX                            # and one along an image edge
        idx = rng.integers(0, B * H * W, 60)
        target.reshape(-1)[idx] = np.resize(np.asarray([-1, K, 200], np.int64), idx.size)
        idx = rng.integers(0, B * H * W, 60)
        pred.reshape(-1)[idx] = np.resize(np.asarray([K, K + 1, 255], np.uint8), idx.size)
    return pred, target


_refs = {}


def case_reference(name):
    """contract_counts of a case; computed once and never modified."""
    if name not in _refs:
        (B, H, W, K, d) = CASES[name][0]
        pred, target = case_maps(name)
        _refs[name] = contract_counts(pred, target, K, IGNORE_INDEX, d)
    return _refs[name]
