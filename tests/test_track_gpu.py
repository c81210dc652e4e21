"""Online tracker on the device (bev_native.track_step: k_track_step of csrc/bev_track.hip, one launch per batch, one
wave per sequence) against the library's host entry -- the same procedure (csrc/bev_track.h) run by one worker.
Every comparison is bit for bit: ids, track_out, info and the whole state blob.  The host entry itself is checked
against an independent restatement in tests/test_track_host.py.
"""
import numpy as np
import pytest
import torch

import track_helper as TH
from conftest import PKG  # noqa: F401  (puts the package on the path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
BOUNDS = (0.0, 9.6, 0.0, 6.4)  # 24 x 36 cells of 0.267 m: a peak that moves one cell stays inside a 1 m gate


@pytest.fixture(scope="module")
def nat():
    import bev_native
    bev_native.lib()
    return bev_native


def params(nat, **kw):
    return nat.TrackParams(**dict(TH.DEFAULTS, **kw))


def on_host(nat, pred, cnt, P, S=1, splits=None, st=None):
    st = nat.track_state(P.max_tracks, sequences=S) if st is None else st
    B = len(cnt) // S
    outs, b = [], 0
    for n in splits or [B]:
        sel = np.concatenate([np.arange(s * B + b, s * B + b + n) for s in range(S)])
        outs.append((sel, nat.track_step_host(pred[sel], cnt[sel], P, st, sequences=S)))
        b += n
    return merge(outs, len(cnt)) + (st,)


def on_device(nat, pred, cnt, P, S=1, splits=None, st=None):
    st = nat.track_state(P.max_tracks, DEV, sequences=S) if st is None else st
    B = len(cnt) // S
    dp, dc = torch.from_numpy(pred).to(DEV), torch.from_numpy(cnt).to(DEV)
    outs, b = [], 0
    for n in splits or [B]:
        sel = np.concatenate([np.arange(s * B + b, s * B + b + n) for s in range(S)])
        ix = torch.from_numpy(sel).to(DEV)
        got = nat.track_step(dp[ix], dc[ix], P, st, sequences=S)
        outs.append((sel, tuple(g.cpu().numpy() for g in got)))
        b += n
    return merge(outs, len(cnt)) + (st.cpu().numpy(),)


def merge(outs, n):
    ids, tracks, info = np.zeros((n, 1024), np.int32), np.zeros((n, 1024, 4), F), np.zeros((n, 4), np.int32)
    for sel, (a, b, c) in outs:
        ids[sel], tracks[sel], info[sel] = a, b, c
    return ids, tracks, info


def assert_same(got, want, what=""):
    for name, a, b in zip(("ids", "tracks", "info", "state"), got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:5])


def both(nat, frames, P, S=1, splits=None, cap=None):
    pred, cnt = TH.pack_frames(frames, cap)
    got, want = on_device(nat, pred, cnt, P, S, splits), on_host(nat, pred, cnt, P, S, splits)
    assert_same(got, want, (S, splits))
    return got


def test_scenarios_splits_and_sequences_equal_host_entry(nat):
    P = params(nat)
    frames = TH.walkers()
    whole = both(nat, frames, P)
    assert whole[0][11, :5].tolist() == [0, 5, 4, 2, 3] and whole[2][9].tolist() == [0, 7, 2, 0]
    for splits in ([1] * 12, [4, 4, 4]):
        assert_same(both(nat, frames, P, splits=splits), whole, splits)
    # three sequences in one launch equal three launches of one
    P7 = params(nat, max_tracks=7, max_age=1)
    seqs = [TH.random_frames(s) for s in (1, 2, 3)]
    got = both(nat, [f for s in seqs for f in s], P7, S=3, cap=7)
    for s, fr in enumerate(seqs):
        one = both(nat, fr, P7, cap=7)
        n = len(fr)
        assert_same(tuple(g[s * n:(s + 1) * n] for g in got[:3]) + (got[3][s:s + 1],), one, s)
    assert_same(both(nat, [f for s in seqs for f in s], P7, S=3, splits=[2, 4], cap=7), got)


@pytest.mark.parametrize("max_age", [0, 2])
def test_size_grid_equals_host_entry(nat, max_age):
    """0, 1, 63, 64, 65 tracks against 0, 1, 64, 65 detections -- one lane short of a wave, a wave, one over -- as 20
    sequences of one launch: frame 0 founds the tracks on a lattice (spacing 0.4, gate 0.5: every neighbour ties),
    frame 1 brings the detections on the lattice shifted by half a cell, frame 2 the first frame again.  max_age 0
    deletes every unmatched track at once (the compaction moves survivors across lanes), 2 keeps them."""
    P = params(nat, gate=0.5, max_age=max_age, max_tracks=130)
    frames, shapes = [], []
    for T in (0, 1, 63, 64, 65):
        for D in (0, 1, 64, 65):
            a, b = TH.lattice(9)[:T], TH.lattice(9, shift=(0.2, 0.0))[::-1][:D].copy()
            frames += [a, b, a]
            shapes.append((T, D))
    ids, tracks, info, st = both(nat, frames, P, S=20, cap=65)
    for s, (T, D) in enumerate(shapes):
        assert info[3 * s].tolist() == [0, T, T, 0], (T, D)
        assert (ids[3 * s + 1, :D] >= 0).all() and (ids[3 * s + 1, D:] == -1).all()  # frame 2 of the warm-up
        assert info[3 * s + 1, 3] == 0 and (max_age == 0 or info[3 * s + 1, 1] == T + info[3 * s + 1, 2])
    v = nat.track_state_view(st, 130)
    assert (v["count"] == info[2::3, 1]).all() and v["count"].max() >= 65


def test_table_limit_lattice_and_truncation_equal_host_entry(nat):
    """1024 x 1024 on a lattice with spacing 0.4 -- the last index of every LDS array, 16 tracks and columns per lane,
    every track with equidistant partners -- and a frame of 1025 detections: its first 1024 are tracked."""
    n = nat.track_max_frame()
    assert n == 1024
    P = params(nat, gate=0.5, max_tracks=n)
    a, b = TH.lattice(32), TH.lattice(32, shift=(0.2, 0.0))
    ids, tracks, info, st = both(nat, [a, b, a], P)
    assert info.tolist() == [[0, n, n, 0], [0, n, 0, 0], [0, n, 0, 0]]
    assert sorted(ids[1].tolist()) == list(range(n)) and sorted(ids[2].tolist()) == list(range(n))
    pts = TH.lattice(33, spacing=3.0)[:n + 1]
    ids, tracks, info, st = both(nat, [pts, pts[::-1].copy()], P)
    T = nat.TRACK_STATUS_TRUNCATED
    assert info.tolist() == [[T, n, n, 0], [T, n, 0, 1]]  # the reversed frame's first detection is the untracked one
    assert ids[1, 0] == -1 and sorted(ids[1, 1:].tolist()) == list(range(1, n))


def test_small_table_fills_up(nat):
    P = params(nat, max_tracks=64, max_age=1)
    rng = np.random.default_rng(5)
    frames = []
    for t in range(4):
        f = np.zeros((40, 4), F)
        f[:, 0], f[:, 1] = 3.0 * np.arange(40) + rng.normal(0, 0.05, 40), 7.0 * (t % 3)  # rows 0, 7, 14 m, then 0 again
        frames.append(f)
    ids, tracks, info, st = both(nat, frames, P)
    # 40 born; 24 more fill the table, 16 dropped; frame 0's 40 tracks leave and 40 are born; the same again
    assert info[:, 1:].tolist() == [[40, 40, 0], [64, 24, 16], [64, 40, 0], [64, 24, 16]]
    assert ids[1, :24].tolist() == list(range(40, 64)) and (ids[1, 24:40] == -1).all()
    assert nat.track_state_view(st, 64)["next_id"][0] == 128


def test_pending_frame_stalls_and_leaves_the_state(nat):
    P = params(nat)
    frames = TH.walkers()
    pred, cnt = TH.pack_frames(frames)
    whole = on_host(nat, pred, cnt, P)
    held = cnt.copy()
    held[5] = -1
    dst = nat.track_state(P.max_tracks, DEV)
    got = on_device(nat, pred[:3], held[:3], P, st=dst)
    before = got[3].copy()
    got = on_device(nat, pred[3:], held[3:], P, st=dst)   # frames 3, 4 tracked, 5 pending, 6.. stalled
    hst = nat.track_state(P.max_tracks)
    on_host(nat, pred[:3], held[:3], P, st=hst)
    want = on_host(nat, pred[3:], held[3:], P, st=hst)
    assert_same(got, want, "pending")
    assert got[2][:, 0].tolist() == [0, 0, nat.TRACK_STATUS_PENDING] + [nat.TRACK_STATUS_STALLED] * 6
    assert got[3].tobytes() != before.tobytes()
    mid = got[3].copy()
    # a launch that finds the stall: every frame stalled, the state as it was
    got = on_device(nat, pred[6:8], cnt[6:8], P, st=dst)
    assert got[2][:, 0].tolist() == [nat.TRACK_STATUS_STALLED] * 2 and (got[0] == -1).all() and not got[1].any()
    assert got[3].tobytes() == mid.tobytes()
    # a pending first frame: nothing but the stalled word moves
    dst2 = nat.track_state(P.max_tracks, DEV)
    on_device(nat, pred[:5], cnt[:5], P, st=dst2)
    copy = dst2.cpu().numpy().copy()
    got = on_device(nat, pred[5:], held[5:], P, st=dst2)
    assert got[2][:, 0].tolist() == [nat.TRACK_STATUS_PENDING] + [nat.TRACK_STATUS_STALLED] * 6
    copy.view(np.int32)[0, 5] = 1
    assert got[3].tobytes() == copy.tobytes()
    # the replay: first = 2 of the second launch (frame 5), its count now known
    dp, dc = torch.from_numpy(pred[3:]).to(DEV), torch.from_numpy(cnt[3:]).to(DEV)
    ids, tracks, info = (t.cpu().numpy() for t in nat.track_step(dp, dc, P, dst, first=2))
    for a, b in zip((ids[2:], tracks[2:], info[2:], dst.cpu().numpy()), (whole[0][5:], whole[1][5:], whole[2][5:], whole[3])):
        assert a.tobytes() == b.tobytes()


def test_reset_and_bad_state_on_the_device(nat):
    P = params(nat)
    fresh = nat.track_state(P.max_tracks)
    dst = torch.full((2, nat.track_state_bytes(P.max_tracks)), 0xAB, dtype=torch.uint8, device=DEV)
    pred, cnt = TH.pack_frames(TH.walkers()[:2] * 2)
    got = nat.track_step(torch.from_numpy(pred).to(DEV), torch.from_numpy(cnt).to(DEV), P, dst, sequences=2)
    assert got[2].cpu().tolist() == [[nat.TRACK_STATUS_BAD_STATE, 0, 0, 0]] * 4 and (got[0] == -1).all()
    assert (dst == 0xAB).all()
    nat.track_reset(dst, P.max_tracks)
    assert dst[0].cpu().numpy().tobytes() == fresh.tobytes() and dst[1].cpu().numpy().tobytes() == fresh.tobytes()


def test_graph_capture_replays_with_new_detections(nat):
    P = params(nat)
    frames = TH.walkers()
    pred, cnt = TH.pack_frames(frames, cap=5)
    dst = nat.track_state(P.max_tracks, DEV)
    dp, dc = torch.zeros(4, 5, 4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    nat.track_step(dp, dc, P, dst)
    nat.track_reset(dst, P.max_tracks)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = nat.track_step(dp, dc, P, dst)
    nat.track_reset(dst, P.max_tracks)  # whatever the capture did or did not run
    got = []
    for b in range(0, 12, 4):
        dp.copy_(torch.from_numpy(pred[b:b + 4]))
        dc.copy_(torch.from_numpy(cnt[b:b + 4]))
        graph.replay()
        got.append(tuple(o.cpu().numpy() for o in outs))
    got = tuple(np.concatenate([g[k] for g in got]) for k in range(3)) + (dst.cpu().numpy(),)
    assert_same(got, on_host(nat, pred, cnt, P), "graph")


# ---- BEVTracker behind a real decode ---------------------------------------------------------------------------------
def _maps(heat):
    B, _, H, W = heat.shape
    rng = np.random.default_rng(H * W + B)
    offset = rng.random((B, 2, H, W), dtype=F)
    size = (rng.random((B, 2, H, W), dtype=F) + F(1.0)).astype(F)
    return [torch.from_numpy(a).to(DEV) for a in (heat, offset, size)]


DECODE = dict(bounds=BOUNDS, conf_thresh=0.3, nms_dist=1.0)
PEAKS = [(3, 4), (10, 20), (18, 9), (6, 30), (20, 28)]


def _batches():
    """Three batches of two frames: 24 x 36 maps whose five peaks move one column per frame; the second batch's
    first frame is a 96 x 96 plateau -- 9216 candidates, more than the on-chip sort holds -- beside a normal frame."""
    hm = TH.moving_peaks(6, 24, 36, PEAKS, step=(0, 1))
    big = np.zeros((2, 1, 96, 96), F)
    big[0] = 0.5
    big[1, 0, 10, 10] = big[1, 0, 50, 60] = 0.9
    return [_maps(hm[0:2]), _maps(big), _maps(hm[4:6])]


def test_tracker_queues_behind_the_lazy_decode(nat):
    from utils.tracking import BEVTracker
    kw = dict(gate=1.0, max_age=2, min_hits=2, max_tracks=64)
    maps = [_maps(TH.moving_peaks(6, 24, 36, PEAKS, step=(0, 1))[b:b + 2]) for b in (0, 2, 4)]
    lazy, listed, cpu = BEVTracker(**kw), BEVTracker(**kw), BEVTracker(**kw)
    res = []
    for m in maps:
        boxes, _ = nat.decode(*m, lazy=True, **DECODE)
        r = lazy.update(boxes)
        assert not boxes.pending.materialised and not r.settled  # queued behind the decode: nobody waited for it
        eager = nat.decode(*m, **DECODE)[0]
        assert [len(b) for b in eager] == [5, 5]
        res.append((r, boxes, listed.update(eager), cpu.update([b.cpu() for b in eager])))
    assert not any(r[1].pending.materialised for r in res)
    for r, boxes, l, c in res:
        for a, b, d in zip(r.ids, l.ids, c.ids):
            assert a.tolist() == b.tolist() == d.tolist()
        for a, b, d in zip(r.tracks, l.tracks, c.tracks):
            assert a.tobytes() == b.tobytes() == d.tobytes()
        assert r.info.tolist() == l.info.tolist() == c.info.tolist()
        assert not boxes.pending.materialised  # the ids were read from the launch's own outputs
    assert lazy.in_flight == 0
    # five people, five ids, kept from frame to frame (one 0.27 m cell per frame, inside the gate)
    assert sorted(res[0][0].ids[0].tolist()) == [0, 1, 2, 3, 4]
    cell = BOUNDS[3] / 24

    def by_row(m, frame, ids):  # keyed by the map row (from y), which no peak shares and none leaves
        y = nat.decode(*m, **DECODE)[0][frame][:, 1].cpu().numpy()
        return dict(zip(np.floor(y / cell).astype(int).tolist(), ids.tolist()))

    first, last = by_row(maps[0], 0, res[0][0].ids[0]), by_row(maps[2], 1, res[2][0].ids[1])
    assert first == last and sorted(first) == sorted(r for r, _ in PEAKS)
    sa, sb, sc = (t.state_dict()["state"].numpy().tobytes() for t in (lazy, listed, cpu))
    assert sa == sb == sc


def test_stall_and_replay_end_with_the_eager_ids(nat):
    from utils.tracking import BEVTracker
    kw = dict(gate=1.0, max_age=2, min_hits=1, max_tracks=256)
    assert 96 * 96 > nat.lib().bev_decode_max_candidates()
    batches = _batches()
    tracker, ref = BEVTracker(**kw), BEVTracker(**kw)
    res, lazies = [], []
    for m in batches:
        boxes, _ = nat.decode(*m, lazy=True, **DECODE)
        res.append(tracker.update(boxes))
        lazies.append(boxes)
    assert not any(b.pending.materialised for b in lazies)
    want = [ref.update([b.cpu() for b in nat.decode(*m, **DECODE)[0]]) for m in batches]
    assert len(want[1].ids[0]) > 10  # the plateau's survivors
    # reading the first batch replays nothing; reading the second materialises its decode and replays the third too
    assert [i.tolist() for i in res[0].ids] == [i.tolist() for i in want[0].ids] and tracker.in_flight == 2
    assert not lazies[1].pending.materialised and not res[1].settled and not res[2].settled
    assert [i.tolist() for i in res[1].ids] == [i.tolist() for i in want[1].ids]
    assert lazies[1].pending.materialised and tracker.in_flight == 0 and res[2].settled
    assert not lazies[2].pending.materialised
    for r, w in zip(res, want):
        assert [i.tolist() for i in r.ids] == [i.tolist() for i in w.ids]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r.tracks, w.tracks)) and r.info.tolist() == w.info.tolist()
    assert tracker.state_dict()["state"].numpy().tobytes() == ref.state_dict()["state"].numpy().tobytes()
    # and the tracker goes on
    boxes, _ = nat.decode(*batches[2], lazy=True, **DECODE)
    more = tracker.update(boxes)
    assert [i.tolist() for i in more.ids] == [i.tolist() for i in ref.update(list(nat.decode(*batches[2], **DECODE)[0])).ids]


def test_state_dict_resumes_mid_sequence(nat):
    from utils.tracking import BEVTracker
    frames = [torch.from_numpy(f).to(DEV) for f in TH.walkers()]
    a = BEVTracker(**TH.DEFAULTS)
    whole = [a.update(frames[b:b + 4]) for b in (0, 4, 8)]
    b = BEVTracker(**TH.DEFAULTS)
    b.update(frames[:4])
    sd = b.state_dict()
    assert sd["state"].device.type == "cpu" and sd["params"]["max_tracks"] == TH.DEFAULTS["max_tracks"]
    c = BEVTracker(device=DEV)
    c.load_state_dict(sd)
    assert c.params == a.params
    rest = [c.update(frames[s:s + 4]) for s in (4, 8)]
    for r, w in zip(rest, whole[1:]):
        assert [i.tolist() for i in r.ids] == [i.tolist() for i in w.ids]
    assert c.state_dict()["state"].numpy().tobytes() == a.state_dict()["state"].numpy().tobytes()
    c.reset()
    again = c.update(frames[:4])
    assert [i.tolist() for i in again.ids] == [i.tolist() for i in whole[0].ids]
