"""pam_crop_table on the GPU against tests/boxes_ref.crop_table, bit for bit: the per-view clamp, the cap cut, the padding rows, a view
subset, and a table longer than the workgroup."""
import numpy as np
import pytest
import torch

import boxes_ref as B

pytestmark = pytest.mark.gpu

W, H = 360, 288


def random_boxes(G, D, seed):
    rng = np.random.default_rng(seed)
    b = np.zeros((G, D, 5), dtype=np.float32)
    b[..., 0] = rng.uniform(-50, W - 10, (G, D)); b[..., 1] = rng.uniform(-50, H - 10, (G, D))
    b[..., 2] = b[..., 0] + rng.uniform(4, 220, (G, D)); b[..., 3] = b[..., 1] + rng.uniform(4, 220, (G, D))
    b[..., 4] = rng.uniform(0.3, 1.0, (G, D))
    return b


def run(boxes, count, max_dets, cap, views=None, n_views=None):
    from pam import _lib
    dev = torch.device('cuda:0')
    n_views = len(views) if views is not None else (n_views or boxes.shape[0])
    tb, tc = torch.from_numpy(boxes).to(dev), torch.tensor(count, dtype=torch.int32, device=dev)
    tv = torch.tensor(views, dtype=torch.int32, device=dev) if views is not None else None
    out = dict(view_of=torch.full((cap,), -7, dtype=torch.int32, device=dev), slot_of=torch.full((cap,), -7, dtype=torch.int32, device=dev),
               xywh=torch.full((cap, 4), -7.0, dtype=torch.float32, device=dev), n_det=torch.full((n_views,), -7, dtype=torch.int32, device=dev),
               info=torch.full((4,), -7, dtype=torch.int32, device=dev))
    _lib.crop_table(torch.cuda.current_stream().cuda_stream, tb, tc, W, H, max_dets, out['view_of'], out['slot_of'], out['xywh'],
                    out['n_det'], out['info'], views=tv)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ref = B.crop_table(boxes, count, W, H, max_dets, cap, views=views, n_views=n_views)
    for k in ref:
        assert got[k].tobytes() == ref[k].tobytes(), (k, got[k], ref[k])
    return got


@pytest.mark.parametrize('count,info', [((2, 0, 5), [6, 6, 1, 0]), ((4, 4, 4), [8, 12, 2, 0]), ((0, 0, 0), [0, 0, 0, 0])],
                         ids=['clamp-and-pad', 'truncate', 'empty'])
def test_small_tables(count, info):
    """V = 3, max_det_in = 8, max_dets = 4, cap = 8."""
    got = run(random_boxes(3, 8, 1), list(count), max_dets=4, cap=8)
    assert got['info'].tolist() == info
    if count == (0, 0, 0):
        assert got['xywh'].tolist() == [[0.0, 0.0, float(W), float(H)]] * 8 and not got['view_of'].any() and not got['slot_of'].any()


def test_view_subset_reads_the_global_lists():
    got = run(random_boxes(5, 8, 2), [1, 2, 3, 4, 2], max_dets=4, cap=8, views=[3, 4])
    assert got['n_det'].tolist() == [4, 2] and got['view_of'].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]


@pytest.mark.parametrize('cap', [160, 496])
def test_thirty_one_views_and_a_table_longer_than_the_workgroup(cap):
    count = np.random.default_rng(5).integers(0, 11, 31).tolist()
    got = run(random_boxes(31, 16, 3), count, max_dets=16, cap=cap)
    assert got['info'][1] == sum(count) and got['info'][0] == min(sum(count), cap)
    assert sum(count) > 128                              # the total is in neither cap's favour by accident: 160 may cut, 496 pads
