"""Online tracker, host side (no GPU): bev_track_step_host (csrc/bev_track.h run by one worker) against the independent
float64 restatement of tests/track_helper.py, and the entry's own contracts: ties, non-finite detections, a full
table, reporting, argument refusals, batch splits, replay with `first`, several sequences.

Tolerance of the comparison with the helper.  Ids and info are integers: exact.  Positions, velocities and
covariances: the filter does about 20 double operations per track and frame; over 12 frames that is 240 roundings of
at most 2^-53 relative each, about 3e-14 relative, on values of at most 60 (metres) -- below 1e-11 m.  The helper
evaluates the same formulas in another, equally valid order (matrix products), so the bound is set at 1e-9 m: two
orders of magnitude of room, five below the float32 spacing of the reported positions.  track_out is float32: both
sides round a double that agrees to 1e-9 m, so they differ only when that double lies within 1e-9 of a rounding
boundary (spacing ~4e-6 at 50 m: a chance of ~5e-4 per sequence); the fixed seeds here do not.

The comparison is well-posed only when the matching is unique beyond rounding, which the test checks in numpy before
it compares: in every frame the best and the runner-up matching of the same cardinality differ by more than 1e-6 m,
and no pair lies within 1e-3 m of the gate.
"""
import ctypes

import numpy as np
import pytest

import track_helper as TH
from conftest import PKG  # noqa: F401  (puts the package on the path)

F = np.float32
TOL = 1e-9


@pytest.fixture(scope="module")
def nat():
    import bev_native
    bev_native.lib()
    return bev_native


def params(nat, **kw):
    return nat.TrackParams(**dict(TH.DEFAULTS, **kw))


def run_host(nat, frames, P, splits=None, cap=None):
    """The frames through the host entry in launches of the given sizes -> (ids, tracks, info, state)."""
    pred, cnt = TH.pack_frames(frames, cap)
    st = nat.track_state(P.max_tracks)
    outs, b = [], 0
    for n in splits or [len(frames)]:
        outs.append(nat.track_step_host(pred[b:b + n], cnt[b:b + n], P, st))
        b += n
    assert b == len(frames)
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3)) + (st,)


def run_ref(frames, **kw):
    ref = TH.RefTracker(**dict(TH.DEFAULTS, **kw))
    return ref, [ref.step(f) for f in frames]


def compare(nat, frames, P, got, ref, steps):
    ids, tracks, info, st = got
    for b, (f, (rid, rout, rinfo, diag)) in enumerate(zip(frames, steps)):
        k = len(f)
        assert ids[b, :k].tolist() == rid.tolist(), (b, ids[b, :k], rid)
        assert (ids[b, k:] == -1).all() and not tracks[b, k:].any()
        assert info[b].tolist() == list(rinfo), (b, info[b], rinfo)
        assert np.abs(tracks[b, :k].astype(np.float64) - rout.astype(np.float64)).max(initial=0.0) <= TOL, b
    v = nat.track_state_view(st, P.max_tracks)
    n = len(ref.state)
    assert v["count"][0] == n and v["next_id"][0] == ref.next_id and v["frames_seen"][0] == ref.frames
    assert v["stalled"][0] == 0
    table = ref.table()
    for k in TH.RefTracker.FIELDS_F:
        assert np.abs(v[k][0, :n] - table[k]).max(initial=0.0) <= TOL, k
        assert not v[k][0, n:].any(), k
    for k in TH.RefTracker.FIELDS_I:
        assert v[k][0, :n].tolist() == table[k].tolist(), k
        assert not v[k][0, n:].any(), k


def test_walkers_equal_the_restated_tracker(nat):
    frames = TH.walkers()
    P = params(nat)
    ref, steps = run_ref(frames)
    diags = [s[3] for s in steps]
    # well-posed: unique matchings, nothing at the gate, small enough to enumerate
    assert all(d["margin"] > 1e-6 and d["gate_margin"] > 1e-3 for d in diags), diags
    assert max(d["tracks"] for d in diags) <= TH.MAX_ENUM and max(d["dets"] for d in diags) <= TH.MAX_ENUM
    # the scenario holds what it says
    assert diags[7]["greedy_differs"], "frame 7: the nearest-pair-first matching is not the optimal one"
    ids = [s[0].tolist() for s in steps]
    infos = [s[2] for s in steps]
    assert ids[0] == [0, 1, 2, 3] and infos[0] == (0, 4, 4, 0)  # warm-up: new tracks are reported
    assert infos[4] == (0, 4, 0, 0) and infos[5] == (0, 4, 1, 0)  # w1's track dies at 5 as w2 is born (id 4)
    # frame 6: w0 is matched again after exactly max_age misses (no birth for it) but its streak restarted; w1 founds
    # a new track; frame 7 shows both: w0 under its id, w1 under a new one -- the dead id 1 is not reused
    assert ids[6] == [-1, -1, 4, 2, 3] and infos[6] == (0, 5, 1, 0)
    assert ids[7] == [0, 5, 4, 2, 3]                              # and no swap at the step of w3 / w4
    assert 1 not in [i for f in ids[5:] for i in f]
    assert len(frames[8]) == 0 and infos[8] == (0, 5, 0, 0)
    assert ids[9] == [-1, -1] and infos[9] == (0, 7, 2, 0)        # only unmatched detections
    assert ids[10] == [-1] * 5 and infos[10] == (0, 7, 0, 0) and ids[11] == [0, 5, 4, 2, 3]  # all picked up again
    compare(nat, frames, P, run_host(nat, frames, P), ref, steps)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_crowds_equal_the_restated_tracker(nat, seed):
    """People within reach of each other's gates, misses and clutter; seeds whose matchings are unique beyond 1e-6."""
    frames = TH.random_frames(seed)
    kw = dict(max_tracks=7, max_age=1)
    ref, steps = run_ref(frames, **kw)
    diags = [s[3] for s in steps]
    assert all(d["margin"] > 1e-6 and d["gate_margin"] > 1e-3 for d in diags), diags
    assert max(d["tracks"] for d in diags) <= TH.MAX_ENUM
    P = params(nat, **kw)
    compare(nat, frames, P, run_host(nat, frames, P), ref, steps)


def test_splits_give_identical_bytes(nat):
    frames = TH.walkers()
    P = params(nat)
    whole = run_host(nat, frames, P, [12])
    for splits in ([1] * 12, [4, 4, 4], [5, 7]):
        part = run_host(nat, frames, P, splits)
        for a, b in zip(whole, part):
            assert a.tobytes() == b.tobytes(), splits


def test_capacity_of_the_pred_buffer_does_not_matter(nat):
    frames = TH.walkers()
    P = params(nat)
    a, b = run_host(nat, frames, P), run_host(nat, frames, P, cap=40)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # a count above cap reads cap rows
    pred, cnt = TH.pack_frames([frames[0][:2]], cap=2)
    st = nat.track_state(P.max_tracks)
    ids, _, info = nat.track_step_host(pred, np.asarray([9], np.int32), P, st)
    assert ids[0, :3].tolist() == [0, 1, -1] and info[0].tolist() == [0, 2, 2, 0]


def test_first_replay_equals_the_uninterrupted_run(nat):
    frames = TH.walkers()
    P = params(nat)
    whole = run_host(nat, frames, P)
    pred, cnt = TH.pack_frames(frames)
    held = cnt.copy()
    held[5] = -1  # frame 5 awaits its decode
    st = nat.track_state(P.max_tracks)
    ids, tracks, info = nat.track_step_host(pred, held, P, st)
    assert info[:, 0].tolist() == [0] * 5 + [nat.TRACK_STATUS_PENDING] + [nat.TRACK_STATUS_STALLED] * 6
    assert (ids[5:] == -1).all() and not tracks[5:].any() and not info[5:, 1:].any()
    v = nat.track_state_view(st, P.max_tracks)
    assert v["stalled"][0] == 1 and v["frames_seen"][0] == 5
    mid = st.copy()
    # a further launch finds the stall: every frame STALLED, not a byte of the state moves
    ids2, _, info2 = nat.track_step_host(pred[6:8], cnt[6:8], P, st)
    assert info2[:, 0].tolist() == [nat.TRACK_STATUS_STALLED] * 2 and (ids2 == -1).all()
    assert st.tobytes() == mid.tobytes()
    # the replay: the same launch from frame 5 on, its count now known
    ids3, tracks3, info3 = nat.track_step_host(pred, cnt, P, st, first=5)
    ids[5:], tracks[5:], info[5:] = ids3[5:], tracks3[5:], info3[5:]
    for a, b in zip(whole, (ids, tracks, info, st)):
        assert a.tobytes() == b.tobytes()
    # first == B: nothing is tracked, the stall is cleared
    st2 = mid.copy()
    nat.track_step_host(pred[:5], cnt[:5], P, st2, first=5)
    assert nat.track_state_view(st2, P.max_tracks)["stalled"][0] == 0
    st2.view(np.int32)[0, 5] = 1
    assert st2.tobytes() == mid.tobytes()


def test_sequences_equal_single_runs(nat):
    P = params(nat, max_tracks=7, max_age=1)
    seqs = [TH.random_frames(s) for s in (1, 2, 3)]
    packed = [TH.pack_frames(f, cap=7) for f in seqs]
    pred, cnt = np.concatenate([p[0] for p in packed]), np.concatenate([p[1] for p in packed])
    st = nat.track_state(P.max_tracks, sequences=3)
    ids, tracks, info = nat.track_step_host(pred, cnt, P, st, sequences=3)
    for s, f in enumerate(seqs):
        one = run_host(nat, f, P, cap=7)
        n = len(f)
        for a, b in zip(one, (ids[s * n:(s + 1) * n], tracks[s * n:(s + 1) * n], info[s * n:(s + 1) * n], st[s:s + 1])):
            assert a.tobytes() == b.tobytes(), s
    assert len({st[s].tobytes() for s in range(3)}) == 3


def frame(*pts):
    f = np.zeros((len(pts), 4), F)
    if pts:
        f[:, :2] = np.asarray(pts, F)
    return f


def test_tie_goes_to_the_lower_detection_index(nat):
    """Two detections at the same float32 distance from one track: the solver's (k, s, column) order takes the lower
    column, the other founds a track; repeatable."""
    P = params(nat)
    frames = [frame((1.0, 1.0)), frame((1.5, 1.0), (0.5, 1.0)), frame((0.5, 1.0), (1.5, 1.0))]
    runs = [run_host(nat, frames, P) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()
    ids, tracks, info, st = runs[0]
    assert ids[0, :1].tolist() == [0]
    assert ids[1, :2].tolist() == [0, 1] and info[1].tolist() == [0, 2, 1, 0]  # detection 0 (x = 1.5) took track 0
    assert tracks[1, 0, 0] > 1.0
    # frame 2: each track has its own detection nearby, in the other order
    assert ids[2, :2].tolist() == [1, 0]
    # and a lattice: four tracks, four detections shifted half a cell, every track with two equidistant partners
    lat = [TH.lattice(2), TH.lattice(2, shift=(0.2, 0.0))]
    a, b = run_host(nat, lat, P), run_host(nat, lat, P)
    assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert sorted(a[0][1, :4].tolist()) == [0, 1, 2, 3] and a[2][1].tolist() == [0, 4, 0, 0]


def test_non_finite_detections_neither_match_nor_found(nat):
    P = params(nat, gate=np.inf)
    nan, inf = np.nan, np.inf
    frames = [frame((0.0, 0.0), (nan, 1.0), (2.0, inf), (4.0, 4.0)),
              frame((nan, nan), (0.1, 0.0), (-inf, 0.0), (4.0, 4.1), (inf, inf))]
    ids, tracks, info, st = run_host(nat, frames, P)
    assert ids[0, :4].tolist() == [0, -1, -1, 1] and info[0].tolist() == [0, 2, 2, 0]
    assert ids[1, :5].tolist() == [-1, 0, -1, 1, -1] and info[1].tolist() == [0, 2, 0, 0]
    assert np.isfinite(tracks).all()
    v = nat.track_state_view(st, P.max_tracks)
    assert all(np.isfinite(v[k]).all() for k in TH.RefTracker.FIELDS_F)


def test_full_table_drops_and_max_tracks_one(nat):
    P = params(nat, max_tracks=3)
    far = [(10.0 * i, 0.0) for i in range(5)]
    frames = [frame(*far), frame(*far)]
    ids, _, info, st = run_host(nat, frames, P)
    assert ids[0, :5].tolist() == [0, 1, 2, -1, -1] and info[0].tolist() == [0, 3, 3, 2]
    assert ids[1, :5].tolist() == [0, 1, 2, -1, -1] and info[1].tolist() == [0, 3, 0, 2]
    assert nat.track_state_view(st, 3)["next_id"][0] == 3  # a dropped detection takes no id
    assert st.shape[1] == nat.track_state_bytes(3) == 256  # 32 + 72 * 3 = 248, rounded up to 16: 8 bytes of padding
    assert not st[0, 248:].any()
    P1 = params(nat, max_tracks=1, max_age=0)
    frames = [frame((0.0, 0.0), (5.0, 5.0)), frame((5.0, 5.0)), frame((5.0, 5.1), (0.0, 0.0))]
    ids, _, info, st = run_host(nat, frames, P1)
    assert ids[0, :2].tolist() == [0, -1] and info[0].tolist() == [0, 1, 1, 1]
    assert ids[1, :1].tolist() == [1] and info[1].tolist() == [0, 1, 1, 0]  # track 0 missed and left; room again
    assert ids[2, :2].tolist() == [1, -1] and info[2].tolist() == [0, 1, 0, 1]
    assert st.shape[1] == 112 and not st[0, 104:].any()


def test_warm_up_and_min_hits_reporting(nat):
    P = params(nat, min_hits=3, max_age=3)
    a = [(0.1 * t, 0.0) for t in range(8)]
    frames = [frame(a[0]), frame(a[1]), frame(a[2]), frame(a[3], (9.0, 9.0)), frame(a[4], (9.0, 9.0)),
              frame(a[5], (9.0, 9.0)), frame((9.0, 9.0)), frame(a[7], (9.0, 9.0))]
    ids, tracks, info, st = run_host(nat, frames, P)
    assert [ids[b, 0] for b in range(6)] == [0] * 6          # frames 1..3 warm-up, then streak >= 3
    assert [ids[b, 1] for b in (3, 4, 5)] == [-1, -1, 1]     # born after the warm-up: shown at its third match
    assert not tracks[3, 1].any() and tracks[5, 1, 0] == pytest.approx(9.0)
    assert ids[6, 0] == 1 and ids[7, :2].tolist() == [-1, 1]  # a miss resets the streak: matched but not shown
    v = nat.track_state_view(st, P.max_tracks)
    assert v["streak"][0, :2].tolist() == [1, 5] and v["age"][0, :2].tolist() == [8, 5]


def test_truncated_frame_tracks_its_first_1024(nat):
    n = nat.track_max_frame()
    assert n == 1024
    pts = TH.lattice(33, spacing=3.0)[:n + 1]
    P = params(nat, max_tracks=1024)
    ids, _, info, _ = run_host(nat, [pts, pts[:n]], P)
    assert info[0].tolist() == [nat.TRACK_STATUS_TRUNCATED, n, n, 0] and ids[0].tolist() == list(range(n))
    assert info[1].tolist() == [0, n, 0, 0] and ids[1].tolist() == list(range(n))


def test_python_refuses_bad_parameters(nat):
    good = dict(TH.DEFAULTS)
    nat.TrackParams(**good)
    for bad in (dict(gate=-1.0), dict(gate=np.nan), dict(q_pos=-1e-9), dict(q_vel=np.inf), dict(r=0.0), dict(r=np.nan),
                dict(p0_vel=-1.0), dict(max_age=-1), dict(min_hits=0), dict(max_tracks=0), dict(max_tracks=1025),
                dict(max_age=1.5)):
        with pytest.raises(ValueError):
            nat.TrackParams(**dict(good, **bad))
    with pytest.raises(ValueError):
        nat.track_state_bytes(0)
    with pytest.raises(ValueError):
        nat.track_state(1025)
    P = params(nat)
    with pytest.raises(ValueError):
        nat.track_step_host(np.zeros((2, 3, 4), F), np.zeros(3, np.int32), P, nat.track_state(P.max_tracks))
    with pytest.raises(ValueError):
        nat.track_step_host(np.zeros((2, 3, 4), F), np.zeros(2, np.int32), P, nat.track_state(P.max_tracks - 1))


def test_c_entry_refuses_before_it_starts(nat):
    L = nat.lib()
    P = params(nat)
    M = P.max_tracks
    nbytes = nat.track_state_bytes(M)
    st = nat.track_state(M)
    pred, cnt = TH.pack_frames(TH.walkers()[:2])
    ids, out, info = np.zeros((2, 1024), np.int32), np.zeros((2, 1024, 4), F), np.zeros((2, 4), np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def call(entry="host", **kw):
        a = dict(pred=p(pred), cnt=p(cnt), S=1, B=2, cap=pred.shape[1], first=0, P=P.c_struct(), st=p(st),
                 stride=nbytes, ids=p(ids), out=p(out), info=p(info))
        a.update(kw)
        args = [a[k] for k in "pred cnt S B cap first P st stride ids out info".split()]
        return L.bev_track_step_host(*args) if entry == "host" else L.bev_track_step_f32(*args, None)

    before = st.copy()
    assert call(B=0) == 0 and call(S=0) == 0 and st.tobytes() == before.tobytes()

    def with_(**kw):
        c = P.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    bad = [dict(pred=None), dict(cnt=None), dict(st=None), dict(ids=None), dict(out=None), dict(info=None),
           dict(B=-1), dict(S=-1), dict(cap=-1), dict(B=65537), dict(first=-1), dict(first=3),
           dict(st=ctypes.c_void_p(st.ctypes.data + 8)), dict(stride=nbytes - 16), dict(stride=nbytes + 8),
           dict(P=with_(max_tracks=0)), dict(P=with_(max_tracks=1025)), dict(P=with_(max_tracks=M + 1)),
           dict(P=with_(thr32=-1.0)), dict(P=with_(thr32=np.nan)), dict(P=with_(q_pos=-1.0)),
           dict(P=with_(q_vel=np.inf)), dict(P=with_(r=0.0)), dict(P=with_(r=np.nan)), dict(P=with_(p0_vel=np.nan)),
           dict(P=with_(max_age=-1)), dict(P=with_(min_hits=0))]
    for kw in bad:
        # both entries answer before any work: the device entry is called with these host pointers, which it never
        # dereferences and never hands to a launch
        assert call(**kw) == nat.BEV_ERR_ARGS, kw
        assert call("device", **kw) == nat.BEV_ERR_ARGS, kw
    assert st.tobytes() == before.tobytes() and not ids.any()
    assert call("device", B=0) == 0 and call("device", S=0) == 0
    assert call(first=2) == 0  # first == B is allowed
    # the reset entries
    assert L.bev_track_state_bytes(0) == nat.BEV_ERR_ARGS and L.bev_track_state_bytes(1025) == nat.BEV_ERR_ARGS
    assert L.bev_track_state_bytes(1) == 112 and L.bev_track_state_bytes(1024) == 32 + 72 * 1024
    for entry, tail in ((L.bev_track_reset_host, ()), (L.bev_track_reset, (None,))):
        assert entry(None, M, *tail) == nat.BEV_ERR_ARGS
        assert entry(p(st), 0, *tail) == nat.BEV_ERR_ARGS and entry(p(st), 1025, *tail) == nat.BEV_ERR_ARGS
        assert entry(ctypes.c_void_p(st.ctypes.data + 4), M, *tail) == nat.BEV_ERR_ARGS


def test_a_blob_that_was_never_reset_is_a_status(nat):
    P = params(nat)
    pred, cnt = TH.pack_frames(TH.walkers()[:2])
    for spoil in ("zeros", "other_size", "count"):
        st = nat.track_state(P.max_tracks)
        if spoil == "zeros":
            st[:] = 0
        elif spoil == "other_size":
            st.view(np.int32)[0, 1] = P.max_tracks + 1
        else:
            st.view(np.int32)[0, 2] = P.max_tracks + 1
        before = st.copy()
        ids, tracks, info = nat.track_step_host(pred, cnt, P, st)
        assert info.tolist() == [[nat.TRACK_STATUS_BAD_STATE, 0, 0, 0]] * 2 and (ids == -1).all() and not tracks.any()
        assert st.tobytes() == before.tobytes()


def test_reset_host_empties_a_used_state(nat):
    P = params(nat)
    frames = TH.walkers()
    fresh = nat.track_state(P.max_tracks)
    *_, st = run_host(nat, frames, P)
    assert st.tobytes() != fresh.tobytes()
    nat.track_reset(st, P.max_tracks)
    assert st.tobytes() == fresh.tobytes()
    v = nat.track_state_view(st, P.max_tracks)
    assert (v["count"][0], v["next_id"][0], v["frames_seen"][0], v["stalled"][0]) == (0, 0, 0, 0)


def test_tracker_class_on_the_cpu_and_save_tracks_json_round_trip(nat, tmp_path):
    import json

    import torch
    from utils.tracking import BEVTracker
    from utils.visualization import save_tracks_json
    frames = TH.walkers()
    P = params(nat)
    want = run_host(nat, frames, P)
    tracker = BEVTracker(**TH.DEFAULTS)
    boxes = [torch.from_numpy(f) for f in frames]
    boxes[8] = None  # the empty frame, as a loader may hand it over
    res = [tracker.update(boxes[b:b + 4]) for b in (0, 4, 8)]
    assert tracker.in_flight == 0 and all(r.settled for r in res)
    ids = [i for r in res for i in r.ids]
    for b, f in enumerate(frames):
        assert ids[b].dtype == np.int32 and ids[b].tolist() == want[0][b, :len(f)].tolist()
    assert np.concatenate([r.info for r in res]).tolist() == want[2].tolist()
    sd = tracker.state_dict()
    assert sd["state"].numpy().tobytes() == want[3].tobytes() and sd["params"] == dict(P._asdict())
    # resume mid-sequence from a state_dict
    a = BEVTracker(**TH.DEFAULTS)
    a.update(boxes[:6])
    b = BEVTracker()
    b.load_state_dict(a.state_dict())
    assert [i.tolist() for i in b.update(boxes[6:]).ids] == [i.tolist() for i in ids[6:]]
    b.reset()
    assert [i.tolist() for i in b.update(boxes[:4]).ids] == [i.tolist() for i in ids[:4]]
    with pytest.raises(ValueError):
        BEVTracker(gate=-1.0)
    with pytest.raises(ValueError):
        b.load_state_dict({"state": sd["state"][:, :-16], "params": sd["params"]})
    # the files: the reference's frame_{idx:06d}.json plus "track_ids"
    scores = [torch.linspace(0.9, 0.5, len(f)) for f in frames]
    paths = save_tracks_json(boxes[:4], scores[:4], ids[:4], str(tmp_path), [7, 8, 9, 10])
    assert [p.rsplit("/", 1)[1] for p in paths] == [f"frame_{i:06d}.json" for i in (7, 8, 9, 10)]
    for b, path in enumerate(paths):
        rec = json.load(open(path))
        assert sorted(rec) == ["boxes", "frame_idx", "scores", "track_ids"] and rec["frame_idx"] == 7 + b
        assert rec["track_ids"] == ids[b].tolist() and rec["boxes"] == frames[b].tolist()
        assert rec["scores"] == scores[b].tolist()
    with pytest.raises(ValueError):
        save_tracks_json(boxes[:1], scores[:1], [ids[1][:1]], str(tmp_path), [0])
