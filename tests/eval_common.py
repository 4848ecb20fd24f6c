"""What the tests of the fusing evaluation modes share (tests/test_tta_gpu.py, tests/test_slide_gpu.py and their references): the top-2 margin of a fused map, and one
eval_base run on the synthetic set with random weights."""
import os

import numpy as np
import torch


def top2_margin(fused):
    """Per pixel, the largest value of fused [B,K,H,W] minus the second largest (inf for K = 1): labels are compared only where the reference itself is that sure."""
    top = fused.topk(min(2, fused.shape[1]), dim=1).values
    return top[:, 0] - top[:, 1] if top.shape[1] == 2 else torch.full_like(top[:, 0], float('inf'))


EVAL_ARGS = ['--model', 'pspnet_pop', '--backbone', 'resnet50', '--dataset', 'synthetic', '--base-size', '128,128', '--restore-from', '/nonexistent', '--allow-random-init',
             '--random-seed', '123']


def run_eval(out, extra, ft=False):
    """eval_base.main with EVAL_ARGS + extra, results under `out` -> the confusion matrix it saved."""
    from segland_amd import eval_base
    torch.manual_seed(0)
    res = eval_base.main(EVAL_ARGS + ['--save-path', str(out)] + extra, ft=ft)
    assert 123 in res
    return np.load(os.path.join(str(out), 'cmatrix_123.npy'))
