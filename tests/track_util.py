"""Point tracks (gpc_hip_track_*), restated plainly: the definitions of include/gpc_hip.h with dicts and loops, for the
tests to hold the GPU result equal to.  Nothing here is clever and nothing here is fast."""
import numpy as np

CORR = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("tar_x", "<i4"), ("tar_y", "<i4")])
TRACK = np.dtype([("first_pair", "<i4"), ("first_record", "<i4"), ("length", "<i4"), ("last_record", "<i4")])


def corr_array(pairs, cap=None):
    """[[(sx, sy, tx, ty), ...] per pair] -> (records [P, cap] of CORR, counts [P]); unused slots hold -9"""
    cap = cap or max(1, max(len(p) for p in pairs))
    rec = np.full((len(pairs), cap, 4), -9, np.int32)
    for t, p in enumerate(pairs):
        for i, r in enumerate(p[:cap]):
            rec[t, i] = r
    return rec.view(CORR).reshape(len(pairs), cap), np.array([len(p) for p in pairs], np.int32)


def restate(rec, counts, W, H):
    """-> (next: list per pair of m_t ints, track_id: the same, rows: list of (first_pair, first_record, length,
    last_record), n_tracks)"""
    P, cap = rec.shape
    m = [min(max(int(counts[t]), 0), cap) for t in range(P)]
    sx, sy, tx, ty = (rec[f].tolist() for f in ("src_x", "src_y", "tar_x", "tar_y"))

    def takes_part(t, i):
        return 0 <= sx[t][i] < W and 0 <= sy[t][i] < H and 0 <= tx[t][i] < W and 0 <= ty[t][i] < H

    nxt = [[-1] * m[t] for t in range(P)]
    for t in range(P - 1):
        lowest_source = {}                       # source pixel of pair t + 1 -> its lowest record
        for j in range(m[t + 1]):
            if takes_part(t + 1, j):
                pix = sy[t + 1][j] * W + sx[t + 1][j]
                if pix not in lowest_source:
                    lowest_source[pix] = j
        candidate = [-1] * m[t]
        winner = {}                              # J -> the lowest i of pair t that wants it
        for i in range(m[t]):
            if takes_part(t, i):
                pix = ty[t][i] * W + tx[t][i]
                if pix in lowest_source:
                    candidate[i] = lowest_source[pix]
                    if candidate[i] not in winner:
                        winner[candidate[i]] = i
        for i in range(m[t]):
            if candidate[i] >= 0 and winner[candidate[i]] == i:
                nxt[t][i] = candidate[i]
    has_pred = [[False] * m[t] for t in range(P)]
    for t in range(P - 1):
        for i in range(m[t]):
            if nxt[t][i] >= 0:
                assert not has_pred[t + 1][nxt[t][i]]
                has_pred[t + 1][nxt[t][i]] = True
    tid = [[-1] * m[t] for t in range(P)]
    rows = []
    for t in range(P):
        for i in range(m[t]):
            if has_pred[t][i]:
                continue
            k, tt, ii, length = len(rows), t, i, 0
            while True:
                tid[tt][ii] = k
                length += 1
                if nxt[tt][ii] < 0:
                    break
                tt, ii = tt + 1, nxt[tt][ii]
            rows.append((t, i, length, ii))
    assert all(v >= 0 for row in tid for v in row)
    return nxt, tid, rows, len(rows)


def expected_arrays(rec, counts, W, H, fill, track_cap):
    """the restatement as the arrays a call leaves in outputs that held `fill` everywhere: (next [P, cap], track_id
    [P, cap], rows [track_cap] of TRACK, n_tracks)"""
    P, cap = rec.shape
    nxt, tid, rows, n = restate(rec, counts, W, H)
    a = np.full((P, cap), fill, np.int32)
    b = np.full((P, cap), fill, np.int32)
    for t in range(P):
        a[t, :len(nxt[t])] = nxt[t]
        b[t, :len(tid[t])] = tid[t]
    tab = np.full((max(track_cap, 1), 4), fill, np.int32)
    for k, r in enumerate(rows[:track_cap]):
        tab[k] = r
    return a, b, tab.view(TRACK).reshape(-1)[:track_cap], n


def track_points(rec, nxt, rows):
    """[(first frame, [(x, y), ...])] per track: the source of every record on the chain, then the last record's target"""
    out = []
    for (t, i, length, last) in rows:
        pts = []
        for k in range(length):
            r = rec[t + k, i]
            pts.append((int(r["src_x"]), int(r["src_y"])))
            if k == length - 1:
                pts.append((int(r["tar_x"]), int(r["tar_y"])))
            else:
                i = nxt[t + k][i]
        out.append((t, pts))
    return out


def fnv_points(tracks):
    """FNV-1a 64 over the int32 (first frame, number of points, x, y, x, y, ...) of every track, in order"""
    h = 1469598103934665603
    for first, pts in tracks:
        words = [first, len(pts)] + [v for p in pts for v in p]
        for b in np.asarray(words, "<i4").tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def frames_of(W, H, N, seed, dy=12):
    """N crops of one seeded texture at offsets that move in x and y (the construction of tests/test_gpu_sequence.py, which
    is dy = 12).  dy = 0 keeps every crop on the same rows: full vertical overlap, so that the epipolar matchers (which
    match within a row only) find the same point in consecutive pairs."""
    rng = np.random.default_rng(seed)
    BW, BH = W + 8 * N + 32, H + 40
    noise = rng.integers(0, 64, (BH, BW))
    base = (rng.integers(0, 256, (BH // 4 + 1, BW // 4 + 1)).repeat(4, 0).repeat(4, 1)[:BH, :BW] * 3 // 4 + noise).astype(np.uint8)
    out = []
    x, y = 16, 20
    for t in range(N):
        out.append(base[y:y + H, x:x + W])
        x += int(rng.integers(1, 8))
        y = 20 + int(rng.integers(-dy, dy + 1))
    return np.ascontiguousarray(np.stack(out))


def oracle_sequence(oracle, frames, forest, epipolar, hashtable, naive=False):
    """the oracle's records of every consecutive pair as (records [P, cap] of CORR, counts [P], candidates per frame)"""
    N, H, W = frames.shape
    pre, codes = [], []
    for f in frames:
        if naive:
            s, gr, m = oracle.preprocess_naive(f, 5)
            codes.append(oracle.hash_naive(s, m, forest))
        else:
            s, gr, m = oracle.preprocess(f, 5)
            codes.append(oracle.hash(s, gr, forest))
        pre.append(m)
    desc = [oracle.descriptors(codes[k], pre[k], W, epipolar) for k in range(N)]
    match = oracle.hash_correspondences if hashtable else oracle.find_correspondences
    want = [match(desc[t], pre[t], desc[t + 1], pre[t + 1], W) for t in range(N - 1)]
    cap = max(1, max(len(w) for w in want))
    rec = np.zeros((N - 1, cap), CORR)
    for t, w in enumerate(want):
        for a, b in (("src_x", "sx"), ("src_y", "sy"), ("tar_x", "tx"), ("tar_y", "ty")):
            rec[a][t, :len(w)] = w[b]
    return rec, np.array([len(w) for w in want], np.int32), [len(m) for m in pre]


def shape_of_tracks(rows, P):
    """(tracks of length >= 3, tracks that end before the last pair, tracks that start after pair 0)"""
    return (sum(1 for r in rows if r[2] >= 3), sum(1 for r in rows if r[0] + r[2] - 1 < P - 1), sum(1 for r in rows if r[0] > 0))
