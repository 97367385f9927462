"""GPU: the device epoch fold (pt_fold_kernel behind srt_pt_fold_epochs_device / srt_pt_group_fold) across launches.

The drop-in class renders launches of up to srt_pt_max_samples_per_launch samples per pixel and folds each one into an
accumulator on the device, replaying do_trace's epoch means and accumulate's running mean (rays/pathtracer.cpp:195-231).  An
epoch may span launches, so the fold carries the epoch in progress from one launch to the next.  Every check here is against
the oracle's epochs folded by the oracle's accumulate, bit for bit, after every fold: the accumulator holds the running mean of
the epochs completed so far, and a partial epoch stays invisible."""
import numpy as np
import pytest

import _harness as H
from _cases import pt_scene

pytestmark = pytest.mark.gpu

SEED = 11
_ORACLES = {}
_EPOCHS = {}


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def _oracle(name, w, h, depth):
    key = (name, w, h, depth)
    if key not in _ORACLES:
        _ORACLES[key] = H.OraclePT(pt_scene(name), w, h, depth, True)
    return _ORACLES[key]


def oracle_epoch(name, w, h, depth, base, n, rows=None):
    """The oracle's epoch of samples base .. base + n - 1 (rows: only [y0, y1)), cached across the tests of this module."""
    key = (name, w, h, depth, base, n, rows)
    if key not in _EPOCHS:
        _EPOCHS[key] = H.oracle_epoch_mt(_oracle(name, w, h, depth), SEED, base, n, rows)
    return _EPOCHS[key]


def expected_means(name, w, h, depth, base, total, spe, first_k=0, acc=None):
    """[running mean after 0, 1, 2, ... completed epochs] of a render of `total` samples from `base` with epochs of `spe`."""
    return H.oracle_running_means(lambda s, n: oracle_epoch(name, w, h, depth, base + s, n), total, spe, first_k, acc, (h, w, 3))


epochs_through = H.epochs_through


def bits_equal(a, b):
    return bool((np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)).all())


def mismatch(a, b):
    return int((np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)).any(axis=-1).sum())


class Single:
    """One context with its device accumulator (torch tensors on the current stream)."""

    def __init__(self, srt, name, w, h, depth, mode=0):
        import torch

        self.torch = torch
        self.w, self.h = w, h
        self.pt = srt.Pathtracer(0)
        self.pt.set_params(w, h, 1, depth, True)
        self.pt.build_scene(pt_scene(name))
        self.pt.set_camera(pt_scene(name)["camera"])
        self.pt.set_kernel(mode)
        _, per_rank, fpt = self.pt.tile_info()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.acc = torch.zeros(self.pt.accumulator_floats(), dtype=torch.float32, device="cuda")
        self.tiles = torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda")
        self.image = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")

    def launch_and_fold(self, base, n, spe, pos, total, first_k):
        self.pt.render_samples_device(self.stream, SEED, base + pos, n)
        self.pt.fold_epochs_device(self.stream, spe, pos, total, first_k, self.acc.data_ptr())

    def image_now(self):
        self.pt.accumulator_tiles_device(self.stream, self.acc.data_ptr(), self.tiles.data_ptr())
        self.pt.untile_device(self.stream, self.tiles.data_ptr(), self.image.data_ptr())
        self.torch.cuda.synchronize()
        return self.image.cpu().numpy().reshape(self.h, self.w, 3)

    def close(self):
        self.pt.close()


# (launch sizes, samples per epoch, first_k): the render's total is the sum of the launches
SCHEDULES = [
    ((64, 64, 22), 15, 0),
    ((17, 1, 64, 33), 7, 0),
    ((9, 6), 1, 0),                        # every sample is an epoch
    ((64, 64, 64, 8), 100, 0),             # an epoch spans two and three launches
    ((64, 64, 64, 64, 44), 200, 0),        # an epoch spans four launches; the short last one spans a launch boundary
    ((30, 20), 9, 1000),                   # Add Samples deep into an accumulator
]


@pytest.mark.parametrize("name,mode", [("cbox", 0), ("cbox", 2), ("cbox", 5), ("cbox_blob512_glass", 6), ("cbox_blob512_glass", 7),
                                       ("cbox_nolight", 0)])
def test_fold_schedules_single_context(srt, name, mode):
    w, h, depth = 40, 28, 6                # two tiles of 32 x 32, padding pixels in both
    one = Single(srt, name, w, h, depth, mode)
    base = 3
    for launches, spe, first_k in SCHEDULES:
        total = sum(launches)
        want = expected_means(name, w, h, depth, base, total, spe, first_k)
        one.acc.zero_()
        pos = 0
        for n in launches:
            one.launch_and_fold(base, n, spe, pos, total, first_k)
            pos += n
            got = one.image_now()
            k = epochs_through(pos, total, spe)
            assert bits_equal(got, want[k]), f"mode {mode}, launches {launches}, spe {spe}: after {pos} samples " \
                                             f"{mismatch(got, want[k])} pixels differ from the running mean of {k} epochs"
        base += total
    one.close()


def test_lane_per_pixel_kernel_is_refused(srt):
    one = Single(srt, "cbox", 16, 16, 4, mode=1)
    with pytest.raises(srt.SrtError) as e:
        one.pt.render_samples_device(one.stream, SEED, 0, 4)
    assert e.value.status == -4                    # SRT_ERR_UNSUPPORTED
    one.close()


def test_add_samples_drops_an_abandoned_partial_epoch(srt):
    """A render cut after a launch that ends mid-epoch leaves the epoch in progress in the accumulator.  The Add Samples render
    that follows (fold at position 0, first_k = the epochs completed) must start from an empty epoch, as the reference drops a
    cancelled partial epoch (rays/pathtracer.cpp:224)."""
    name, w, h, depth = "cbox", 40, 28, 6
    one = Single(srt, name, w, h, depth)
    # render A: 40 samples in epochs of 10, abandoned after its first launch of 25 (two epochs complete, five samples pending)
    one.launch_and_fold(0, 25, 10, 0, 40, 0)
    want_a = expected_means(name, w, h, depth, 0, 20, 10)
    got = one.image_now()
    assert bits_equal(got, want_a[2]), f"{mismatch(got, want_a[2])} pixels"
    # render B (Add Samples): 12 samples in epochs of 5 from sample 40 (begin counts the abandoned render in full), launches 7 + 5
    want_b = expected_means(name, w, h, depth, 40, 12, 5, first_k=2, acc=want_a[2])
    pos = 0
    for n in (7, 5):
        one.launch_and_fold(40, n, 5, pos, 12, 2)
        pos += n
        got = one.image_now()
        k = epochs_through(pos, 12, 5)
        assert bits_equal(got, want_b[k]), \
            f"after {pos} samples of the Add Samples render: {mismatch(got, want_b[k])} pixels differ (the abandoned partial epoch leaked in?)"
    one.close()


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
@pytest.mark.parametrize("w,h", [(72, 40), (24, 16)])      # padding tiles / smaller than a tile: ranks 1 and 2 own nothing
def test_group_two_lanes_in_flight(srt, devices, w, h):
    """RenderCore::worker's schedule on the group ABI: launches alternate lanes 0 and 1, two are enqueued before the first fold,
    folds go in launch order (ordered by events across the lanes' streams)."""
    name, depth, n, spe, base = "cbox", 6, 150, 45, 5
    want = expected_means(name, w, h, depth, base, n, spe)
    g = srt.PathtracerGroup(devices)
    g.set_params(w, h, n, depth, True)
    g.build_scene(pt_scene(name))
    g.set_camera(pt_scene(name)["camera"])
    g.reset_accumulator()
    most = g.max_samples_per_launch()
    assert most == 64
    inflight, nxt, lane, folds = [], 0, 0, 0
    while True:
        while len(inflight) < 2 and nxt < n:
            m = min(most, n - nxt)
            g.render_samples(lane, SEED, base + nxt, m)
            inflight.append((nxt, m, lane))
            nxt += m
            lane ^= 1
        if not inflight:
            break
        pos, m, ln = inflight.pop(0)
        g.wait_lane(ln)
        g.fold(ln, spe, pos, n, 0)
        folds += 1
        got = g.accumulator_image()
        k = epochs_through(pos + m, n, spe)
        assert bits_equal(got, want[k]), f"devices {devices}: after {pos + m} samples {mismatch(got, want[k])} pixels differ"
    assert folds == 3
    g.close()


def test_launch_cap_below_64(srt):
    """4096 x 2048: the per-sample buffer caps a launch at 16 samples per pixel.  One epoch of 40 samples spans three launches
    (16 + 16 + 8) and a short second epoch of 4 follows in the third; 64 random pixels against per-sample radiance
    (srt_pt_trace_samples) folded on the host with do_trace's and accumulate's float arithmetic."""
    name, w, h, depth, base, spe, total = "cbox_lambertian", 4096, 2048, 8, 5, 40, 44
    one = Single(srt, name, w, h, 8)
    assert one.pt.max_samples_per_launch() == 16
    rng = np.random.default_rng(0)
    xs = rng.integers(0, w, 64).astype(np.uint32)
    ys = rng.integers(0, h, 64).astype(np.uint32)
    rgb = np.stack([one.pt.trace_samples(SEED, np.full(total, x, np.uint32), np.full(total, y, np.uint32),
                                         np.arange(base, base + total, dtype=np.uint32))[0] for x, y in zip(xs, ys)])   # [pixel][sample][3]
    means = []
    for s0 in range(0, total, spe):
        e = np.zeros((len(xs), 3), np.float32)
        for p in range(len(xs)):
            acc, cnt = np.zeros(3, np.float32), 0
            for s in range(s0, min(s0 + spe, total)):
                if np.isfinite(rgb[p, s]).all():
                    acc = (acc + rgb[p, s]).astype(np.float32)
                    cnt += 1
            e[p] = (acc * (np.float32(1.0) / np.float32(cnt))).astype(np.float32) if cnt else acc
        means.append(e)
    want = [np.zeros((len(xs), 3), np.float32)]
    for k, e in enumerate(means, 1):
        a = want[-1]
        want.append((a + ((e - a).astype(np.float32) * (np.float32(1.0) / np.float32(k))).astype(np.float32)).astype(np.float32))
    pos = 0
    for n in (16, 16, 12):
        one.launch_and_fold(base, n, spe, pos, total, 0)
        pos += n
        got = one.image_now()[ys, xs]
        k = epochs_through(pos, total, spe)
        assert bits_equal(got, want[k]), f"after {pos} samples: {mismatch(got, want[k])} of 64 pixels differ"
    one.close()


def test_a_cancelled_launch_is_not_folded(srt):
    """srt_pt_cancel while a launch is in flight: the fold behind it on the same stream is skipped, or - if the launch finished
    first - folds all of it.  Anything in between fails.  After srt_pt_clear_cancel a fresh render matches the oracle."""
    name, w, h, depth = "cbox_blob512_glass", 512, 512, 8
    one = Single(srt, name, w, h, depth)
    first = expected_means(name, w, h, depth, 0, 2, 2)
    one.launch_and_fold(0, 2, 2, 0, 66, 0)           # a render of 66 in epochs of 2: the first launch completes one epoch
    before = one.image_now()
    assert bits_equal(before, first[1]), f"{mismatch(before, first[1])} pixels"
    one.pt.render_samples_device(one.stream, SEED, 2, 64)
    one.pt.cancel_device()
    one.pt.fold_epochs_device(one.stream, 2, 2, 66, 0, one.acc.data_ptr())
    got = one.image_now()
    if bits_equal(got, before):
        print("cancelled launch: cut, nothing folded")
    else:
        print("cancelled launch: finished before the cancel, folded in full")
        rows = (0, 8)                                # the oracle of 64 samples on eight rows is enough to tell the two apart
        acc = before.copy()
        for j in range(32):
            H.oracle_accumulate(acc, oracle_epoch(name, w, h, depth, 2 + 2 * j, 2, rows), j + 2)
        assert bits_equal(got[rows[0]:rows[1]], acc[rows[0]:rows[1]]), \
            f"a cancelled launch was folded in part: {mismatch(got[rows[0]:rows[1]], acc[rows[0]:rows[1]])} of {w * 8} pixels differ from both outcomes"
    assert one.pt.cancel_requested()
    one.pt.clear_cancel()
    assert not one.pt.cancel_requested()
    one.acc.zero_()
    one.launch_and_fold(0, 2, 2, 0, 2, 0)
    got = one.image_now()
    assert bits_equal(got, first[1]), f"after clear_cancel: {mismatch(got, first[1])} pixels"
    one.close()
