"""The inputs of the rotation / blur tests, shared by the CPU tests (which bound the near-tie mask and state the float32 error of the reference on exactly these inputs) and the
GPU tests (which run them through the kernel).  Nothing here imports the package; draws are the plain 16-tuples of aug_geo_reference.angle_draw."""
import numpy as np

import aug_geo_reference as gr
import aug_reference as ar

CH = CW = 32
MEAN = STD = (0.5, 0.5, 0.5)
SIZES = [(40, 56), (37, 53), (64, 64), (20, 28)]           # the last one is smaller than the crop
ANGLES = [7.5, -33.0, 61.3, 135.7, -171.0]                 # 45 and 90 are left out: at scale 0.5 they put 1.2 % and 16.5 % of the pixels on ties
SCALES = [0.5, 0.73, 1.0, 1.37, 2.0]
STRONG = (1.4, 0.2, 1.5)
STRONGEST = (1.99, 0.5, 1.99)
BLUR_SIZES = (3, 5, 7, 9, 11)
LUT = ((np.arange(256) * 7 + 3) % 251).astype(np.uint8)


def tiles(seed=0, sizes=SIZES, band=3):
    """Random tiles whose labels hold a band of 255."""
    rng = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        lab = rng.randint(0, 12, (h, w)).astype(np.uint8)
        lab[:band] = 255
        out.append((rng.randint(0, 256, (h, w, 3)).astype(np.uint8), lab))
    return out


def rotation_launches(triple):
    """Five launches of 64 crops: in launch n tile t meets scale (n + t) mod 5 and angle (n + 2t) mod 5, so every tile meets every scale and every angle; flip x k x offsets at
    0 and at the far edge of the rescaled tile."""
    for n in range(len(SCALES)):
        draws = []
        for t, (H, W) in enumerate(SIZES):
            s, angle = SCALES[(n + t) % len(SCALES)], ANGLES[(n + 2 * t) % len(ANGLES)]
            Hs, Ws = ar.scaled_size(H, s), ar.scaled_size(W, s)
            for flip in (False, True):
                for k in range(4):
                    for h_off, w_off in ((0, 0), (max(Hs - CH, 0), max(Ws - CW, 0))):
                        draws.append((t, gr.angle_draw(h_off, w_off, flip, k, Hs, Ws, triple, H, angle)))
        yield draws


def blur_launches():
    """(name, crop, [(tile, draw)]): every K on 32 x 32 crops of every tile (the small one included: padding taps), K = 11 on an 8 x 8 crop, K = 5 on a 40 x 24 crop with even
    k, and every K combined with a rotation at scale 0.73 (the last of them with the strong jitter)."""
    for K in BLUR_SIZES:
        draws = []
        for t, (H, W) in enumerate(SIZES):
            for j, (h_off, w_off) in enumerate(((0, 0), (max(H - CH, 0), max(W - CW, 0)))):
                for fk in range(4):
                    draws.append((t, gr.angle_draw(h_off, w_off, bool((fk + j) % 2), (fk + t) % 4, H, W, None, H, None, K)))
        yield 'K=%d' % K, (CH, CW), draws
    yield 'K=11 on 8x8', (8, 8), [(t, gr.angle_draw(o, o + 1, bool(k % 2), k, H, W, None, H, None, 11)) for t, (H, W) in enumerate(SIZES) for k in range(4) for o in (0, 11)]
    yield 'K=5 on 40x24', (40, 24), [(t, gr.angle_draw(o, 2 * o, bool(o), k, H, W, None, H, None, 5)) for t, (H, W) in enumerate(SIZES) for k in (0, 2) for o in (0, 9)]
    draws = []
    for i, K in enumerate(BLUR_SIZES):
        for t, (H, W) in enumerate(SIZES):
            Hs, Ws = ar.scaled_size(H, 0.73), ar.scaled_size(W, 0.73)
            draws.append((t, gr.angle_draw(max(Hs - CH, 0) // 2, max(Ws - CW, 0), bool(t % 2), (t + i) % 4, Hs, Ws, STRONG if K == 11 else None, H, ANGLES[(i + t) % len(ANGLES)], K)))
    yield 'rotation + scale 0.73', (CH, CW), draws
