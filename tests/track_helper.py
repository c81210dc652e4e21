"""Helpers of the tracker tests (tests/test_track_host.py, tests/test_track_gpu.py): a float64 numpy restatement of the
tracker's six steps that is independent of the library -- it imports neither the package nor its bindings and calls no
solver -- and the scenarios both files share.

The definition (csrc/bev_track.h), restated.  A track is (x, y, vx, vy), one covariance (p00, p01, p11) for both axes,
id, streak, misses, age.  Per frame: 1. predict every track (F = [[1, 1], [0, 1]], P <- F P F' + diag(q_pos, q_vel));
2. match tracks at their float32 positions to the detections: a pair is admissible when its float32 distance is <= gate
and finite, the matching has the most pairs and among those the smallest sum; 3. Kalman update of the matched tracks
with H = [1, 0] and measurement variance r, streak += 1, misses = 0, unmatched: streak = 0; 4. drop tracks with
misses > max_age, keeping the order; 5. each unmatched finite detection, in order, founds a track (P = diag(r, p0_vel),
next id) while the table has room, else it is dropped; 6. detection c reports its track's id when the track's
streak >= min_hits or at most min_hits frames were seen, else -1.

The matching here is found by enumerating every matching of the frame (each track takes an admissible unused detection
or none), so a frame may have at most 7 tracks and 7 detections.  The enumeration also yields the runner-up, which is
how a test knows that a comparison with the library is well-posed: RefTracker.step reports, per frame, how far the
best sum is from the best different matching of the same cardinality and how close any pair lies to the gate.
"""
import numpy as np

from mod_metrics_helper import F, admissible, dist32

MAX_ENUM = 7


def matchings(ok):
    """Every set of admissible pairs with distinct rows and columns, as tuples of (row, col)."""
    K, G = ok.shape
    out = []

    def rec(i, used, pairs):
        if i == K:
            out.append(tuple(pairs))
            return
        rec(i + 1, used, pairs)
        for j in range(G):
            if ok[i, j] and not used & (1 << j):
                rec(i + 1, used | (1 << j), pairs + [(i, j)])

    rec(0, 0, [])
    return out


def best_matching(p, g, gate):
    """p [K, 2], g [G, 2] float32 -> (pairs of the matching with the most pairs and the smallest sum, margin: how much
    larger the sum of the best other matching of that cardinality is (inf when there is none), gate_margin: the
    smallest |distance - gate| over all pairs, d32)."""
    K, G = len(p), len(g)
    if K == 0 or G == 0:
        return (), np.inf, np.inf, np.zeros((K, G), F)
    assert K <= MAX_ENUM and G <= MAX_ENUM, "the enumeration is for small frames"
    d = dist32(p, g)
    ok = admissible(d, gate)
    d64 = d.astype(np.float64)
    scored = sorted(((-len(m), float(sum(d64[i, j] for i, j in m)), m) for m in matchings(ok)), key=lambda t: t[:2])
    best = scored[0]
    same = [s for s in scored[1:] if s[0] == best[0]]
    margin = same[0][1] - best[1] if same else np.inf
    with np.errstate(invalid="ignore"):
        gm = np.abs(d64 - gate)
    gate_margin = float(np.nanmin(gm)) if np.isfinite(gm).any() else np.inf
    return best[2], margin, gate_margin, d


def greedy_matching(d, ok):
    """The nearest-pair-first matching: repeatedly the admissible pair of least distance among unused rows / columns."""
    pairs, d = [], np.where(ok, d.astype(np.float64), np.inf)
    while d.size and np.isfinite(d).any():
        i, j = np.unravel_index(np.argmin(d), d.shape)
        pairs.append((int(i), int(j)))
        d[i, :] = np.inf
        d[:, j] = np.inf
    return tuple(sorted(pairs))


class RefTracker:
    """The restated tracker.  Tracks are rows of float64 / int64 arrays in slot order."""
    FIELDS_F = ("x", "y", "vx", "vy", "p00", "p01", "p11")
    FIELDS_I = ("id", "streak", "misses", "age")

    def __init__(self, gate, max_age, min_hits, q_pos, q_vel, r, p0_vel, max_tracks):
        self.gate, self.max_age, self.min_hits, self.max_tracks = float(gate), max_age, min_hits, max_tracks
        self.Q = np.diag([q_pos, q_vel]).astype(np.float64)
        self.r, self.p0_vel = float(r), float(p0_vel)
        self.state = np.zeros((0, 4))   # x, vx, y, vy
        self.cov = np.zeros((0, 2, 2))
        self.ints = np.zeros((0, 4), np.int64)
        self.next_id = self.frames = 0

    def table(self):
        s, c = self.state, self.cov
        out = {"x": s[:, 0], "vx": s[:, 1], "y": s[:, 2], "vy": s[:, 3], "p00": c[:, 0, 0], "p01": c[:, 0, 1],
               "p11": c[:, 1, 1]}
        out.update({k: self.ints[:, i] for i, k in enumerate(self.FIELDS_I)})
        return out

    def step(self, det):
        """det [K, >= 2] float32 -> ids [K], out [K, 4] float32 (x, y, vx, vy), info (0, live, born, dropped), diag."""
        det = np.asarray(det, F).reshape(-1, 4)[:, :2]
        self.frames += 1
        Fm = np.array([[1.0, 1.0], [0.0, 1.0]])
        n = len(self.state)
        # 1. predict
        if n:
            self.state = np.stack([self.state[:, 0] + self.state[:, 1], self.state[:, 1],
                                   self.state[:, 2] + self.state[:, 3], self.state[:, 3]], 1)
            self.cov = np.stack([Fm @ P @ Fm.T + self.Q for P in self.cov])
            self.ints[:, 2] += 1
            self.ints[:, 3] += 1
        # 2. associate
        pos = self.state[:, [0, 2]].astype(F)
        pairs, margin, gate_margin, d = best_matching(pos, det, self.gate)
        greedy = greedy_matching(d, admissible(d, self.gate)) if n and len(det) else ()
        row_of = {j: i for i, j in pairs}
        col_of = dict(pairs)
        # 3. update
        for i in range(n):
            if i not in col_of:
                self.ints[i, 1] = 0
                continue
            z = det[col_of[i]].astype(np.float64)
            P = self.cov[i]
            s = P[0, 0] + self.r
            gain = P[:, 0] / s
            for a in (0, 1):
                e = z[a] - self.state[i, 2 * a]
                self.state[i, 2 * a:2 * a + 2] += gain * e
            self.cov[i] = P - np.outer(gain, P[0, :])
            self.ints[i, 1] += 1
            self.ints[i, 2] = 0
        # 4. delete
        keep = self.ints[:, 2] <= self.max_age
        new_slot = np.cumsum(keep) - 1
        self.state, self.cov, self.ints = self.state[keep], self.cov[keep], self.ints[keep]
        # 5. birth
        slot_of = {j: int(new_slot[i]) for j, i in row_of.items()}
        born = dropped = 0
        for j in range(len(det)):
            if j in row_of or not np.isfinite(det[j]).all():
                continue
            if len(self.state) >= self.max_tracks:
                dropped += 1
                continue
            slot_of[j] = len(self.state)
            self.state = np.vstack([self.state, [[det[j, 0], 0.0, det[j, 1], 0.0]]])
            self.cov = np.concatenate([self.cov, np.diag([self.r, self.p0_vel])[None]])
            self.ints = np.vstack([self.ints, [[self.next_id, 1, 0, 1]]])
            self.next_id += 1
            born += 1
        # 6. report
        ids = np.full(len(det), -1, np.int32)
        out = np.zeros((len(det), 4), F)
        for j, s in slot_of.items():
            if self.ints[s, 1] >= self.min_hits or self.frames <= self.min_hits:
                ids[j] = self.ints[s, 0]
                out[j] = self.state[s, [0, 2, 1, 3]]
        diag = {"margin": margin, "gate_margin": gate_margin, "greedy_differs": tuple(sorted(pairs)) != greedy,
                "tracks": n, "dets": len(det)}
        return ids, out, (0, len(self.state), born, dropped), diag


DEFAULTS = dict(gate=1.0, max_age=2, min_hits=2, q_pos=0.01, q_vel=0.01, r=0.01, p0_vel=0.25, max_tracks=16)
N_FRAMES = 12


def walkers(seed=7, sigma=0.03):
    """12 frames of up to 6 walkers on straight lines with Gaussian jitter (DEFAULTS: max_age 2, gate 1 m):
      w0  misses frames 4, 5 -- exactly max_age -- and is picked up again at 6 under its id;
      w1  misses frames 3, 4, 5 -- max_age + 1 -- so its track dies at 5; at 6 it founds a new one, the id is not reused;
      w2  a newcomer at frame 5;
      w3, w4  walk side by side 0.5 m apart; at frame 7 both step so that the nearest pair is w4's track with w3's
              detection (0.2 m, leaving w3's track a 0.9 m partner) while the optimal matching keeps both (0.3 + 0.4);
      frame 8 is empty; frame 9 holds only two detections 50 m away, which match nothing and found two tracks.
    -> list of [K, 4] float32 (x, y, 0.6, 0.6)."""
    rng = np.random.default_rng(seed)
    start = {0: (0.0, 0.0), 1: (5.0, 0.0), 2: (10.0, 3.0), 3: (20.0, 0.0), 4: (20.5, 0.0)}
    vel = {0: (0.3, 0.05), 1: (0.2, 0.1), 2: (-0.25, 0.1), 3: (0.1, 0.0), 4: (0.1, 0.0)}
    absent = {0: {4, 5}, 1: {3, 4, 5}, 2: {0, 1, 2, 3, 4}, 3: set(), 4: set()}
    frames = []
    for t in range(N_FRAMES):
        rows = []
        if t == 9:
            rows = [(50.0, 50.0), (53.0, 50.0)]
        elif t != 8:
            for w in range(5):
                if t in absent[w]:
                    continue
                x, y = start[w][0] + vel[w][0] * t, start[w][1] + vel[w][1] * t
                if t >= 7 and w == 3:
                    x += 0.3
                if t >= 7 and w == 4:
                    x += 0.4
                rows.append((x + rng.normal(0, sigma), y + rng.normal(0, sigma)))
        f = np.zeros((len(rows), 4), F)
        if rows:
            f[:, :2] = np.asarray(rows)
            f[:, 2:] = 0.6
        frames.append(f)
    return frames


def random_frames(seed, n_frames=6, n_people=5, extent=4.0, sigma=0.05, p_miss=0.2, p_clutter=0.3):
    """A denser random sequence on a small square (people within reach of each other's gates): every person steps
    with its own velocity, is missed with p_miss, and a clutter detection appears with p_clutter.  At most 7
    detections per frame."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, extent, (n_people, 2))
    vel = rng.normal(0, 0.25, (n_people, 2))
    frames = []
    for _ in range(n_frames):
        pos = pos + vel
        rows = [p + rng.normal(0, sigma, 2) for p in pos if rng.random() >= p_miss]
        if rng.random() < p_clutter:
            rows.append(rng.uniform(0, extent, 2))
        rows = [rows[i] for i in rng.permutation(len(rows))][:MAX_ENUM]
        f = np.zeros((len(rows), 4), F)
        if rows:
            f[:, :2] = np.asarray(rows)
        frames.append(f)
    return frames


def pack_frames(frames, cap=None):
    """pred [B, cap, 4] float32 and pred_count [B] int32 (the decode's layout)."""
    ks = [len(f) for f in frames]
    cap = max(ks + [1]) if cap is None else cap
    pred = np.zeros((len(frames), cap, 4), F)
    for b, f in enumerate(frames):
        pred[b, :ks[b]] = f
    return pred, np.asarray(ks, np.int32)


def lattice(n_side, spacing=0.4, shift=(0.0, 0.0)):
    """n_side x n_side points on a square lattice (heavy ties: every neighbour is equidistant), as [n, 4] float32."""
    xs = (np.arange(n_side) * spacing).astype(F)
    pts = np.zeros((n_side * n_side, 4), F)
    pts[:, 0], pts[:, 1] = np.repeat(xs, n_side) + F(shift[0]), np.tile(xs, n_side) + F(shift[1])
    return pts


def moving_peaks(n_frames, H, W, peaks, step=(1, 0), value=0.9):
    """Heatmaps [n_frames, 1, H, W] float32 with isolated one-cell peaks that move `step` cells (row, col) per frame
    (for a real decode): peaks a list of (row, col)."""
    hm = np.zeros((n_frames, 1, H, W), F)
    for t in range(n_frames):
        for k, (r, c) in enumerate(peaks):
            hm[t, 0, (r + step[0] * t) % H, (c + step[1] * t) % W] = value - 0.01 * k
    return hm
