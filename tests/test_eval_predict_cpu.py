"""The three predictors of the evaluation loop (segland_amd/eval_base.py: predict_plain and select_predictor) without a GPU and without the library: the four ops they can
reach are replaced by recorders, the model by a stub, and each predictor must issue exactly its own calls with the sizes it was given.  An 8-channel 4x3 logit on a 16x12
image, scored on the 16x16 long-side square: every size involved differs from the others in at least one side."""
import pytest
import torch

from segland_amd import eval_base, ops

B, K = 2, 8
IMAGE, LOGIT, SCORE = (16, 12), (4, 3), (16, 16)


@pytest.fixture
def calls(monkeypatch):
    """[(op name, args, kwargs), ...] in call order; the recorders return zero tensors of the shapes the ops give."""
    seen = []

    def fused_pair(n, size, want_map):
        return torch.zeros((n,) + tuple(size), dtype=torch.uint8), torch.zeros((n, K) + tuple(size)) if want_map else None

    def upsample_argmax(logits, size):
        seen.append(('upsample_argmax', (tuple(logits.shape), tuple(size)), {}))
        return torch.zeros((logits.shape[0],) + tuple(size), dtype=torch.uint8)

    def upsample_logits(logits, size):
        seen.append(('upsample_logits', (tuple(logits.shape), tuple(size)), {}))
        return torch.zeros(tuple(logits.shape[:2]) + tuple(size))

    def tta_fuse(views, size, mode='prob', want_map=False):
        seen.append(('tta_fuse', ([(tuple(l.shape), f, w) for l, f, w in views], tuple(size)), {'mode': mode, 'want_map': want_map}))
        return fused_pair(views[0][0].shape[0], size, want_map)

    def slide_fuse(logits, n, size, crop, stride, mode='prob', blend='uniform', want_map=False):
        seen.append(('slide_fuse', (tuple(logits.shape), n, tuple(size), tuple(crop), tuple(stride)), {'mode': mode, 'blend': blend, 'want_map': want_map}))
        return fused_pair(n, size, want_map)

    for fn in (upsample_argmax, upsample_logits, tta_fuse, slide_fuse):
        monkeypatch.setattr(ops, fn.__name__, fn)
    return seen


def stub_model(batches):
    """image -> zeros [B,K,4,3]; the batch size of every call is appended to `batches`."""
    def model(image):
        batches.append(image.shape[0])
        return torch.zeros((image.shape[0], K) + LOGIT)
    return model


def select(argv):
    return eval_base.select_predictor(eval_base.get_parser().parse_args(argv))


def image():
    return torch.zeros((B, 3) + IMAGE)


def test_plain_without_a_map(calls):
    batches = []
    labels, out_map = eval_base.predict_plain(stub_model(batches), image(), SCORE)
    assert calls == [('upsample_argmax', ((B, K) + LOGIT, SCORE), {})]
    assert batches == [B] and out_map is None
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B,) + SCORE


def test_plain_with_a_map(calls):
    labels, out_map = eval_base.predict_plain(stub_model([]), image(), SCORE, IMAGE)
    assert calls == [('upsample_argmax', ((B, K) + LOGIT, SCORE), {}), ('upsample_logits', ((B, K) + LOGIT, IMAGE), {})]
    assert tuple(labels.shape) == (B,) + SCORE and tuple(out_map.shape) == (B, K) + IMAGE


@pytest.mark.parametrize('map_size', [None, IMAGE])
def test_tta_predictor(calls, map_size):
    predict, describe = select(['--tta-flip', 'True', '--tta-mode', 'logit'])
    batches = []
    labels, out_map = predict(stub_model(batches), image(), SCORE, map_size)
    view = (B, K) + LOGIT
    assert calls == [('tta_fuse', ([(view, 0, 1.0), (view, 1, 1.0)], SCORE), {'mode': 'logit', 'want_map': map_size is not None})]
    assert batches == [B, B]
    assert tuple(labels.shape) == (B,) + SCORE and (out_map is None) == (map_size is None)
    assert describe(IMAGE, SCORE) == 'test-time augmentation: 2 views per tile (images 16x12; each plain and mirrored), mode logit, fused at 16x16'


@pytest.mark.parametrize('map_size', [None, IMAGE])
def test_sliding_predictor(calls, map_size):
    predict, describe = select(['--slide-crop', '64,64', '--slide-stride', '32,32', '--slide-mode', 'logit', '--slide-blend', 'tent', '--slide-batch', '1'])
    batches = []
    labels, out_map = predict(stub_model(batches), image(), IMAGE, map_size)
    # one 16x12 window per image (the crop is clamped to the tile), forwarded one at a time
    assert calls == [('slide_fuse', ((B, K) + LOGIT, B, IMAGE, (64, 64), (32, 32)), {'mode': 'logit', 'blend': 'tent', 'want_map': map_size is not None})]
    assert batches == [1, 1]
    assert tuple(labels.shape) == (B,) + IMAGE and (out_map is None) == (map_size is None)
    assert describe(IMAGE, IMAGE) == 'sliding-window inference: 1 windows per tile (1 x 1 of 16x12 on 16x12), crop 64x64, stride 32x32, blend tent, mode logit'


def test_sliding_refuses_another_scoring_grid(calls):
    predict, _ = select(['--slide-crop', '64,64'])
    batches = []
    with pytest.raises(ValueError, match='scored at 16x16 but the image is 16x12'):
        predict(stub_model(batches), image(), SCORE)
    assert calls == [] and batches == []


def test_selection(calls):
    predict, describe = select([])
    assert predict is eval_base.predict_plain and describe is None
    predict, describe = select(['--tta-scales', '1.0', '--tta-flip', 'False'])
    assert predict is eval_base.predict_plain and describe is None
    for argv, op, size in ((['--tta-flip', 'True'], 'tta_fuse', SCORE), (['--tta-scales', '0.5'], 'tta_fuse', SCORE), (['--slide-crop', '64,64'], 'slide_fuse', IMAGE)):
        del calls[:]
        predict, describe = select(argv)
        assert describe is not None
        predict(stub_model([]), image(), size)
        assert [c[0] for c in calls] == [op], argv
    with pytest.raises(ValueError, match='--slide-crop together with --tta-scales / --tta-flip'):
        select(['--slide-crop', '64,64', '--tta-flip', 'True'])
    with pytest.raises(ValueError, match='multiples of 32'):
        select(['--slide-crop', '48,64'])
