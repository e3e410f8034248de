"""Shared by the group-mode tests: the packing rule of gpc_hip_parse_forest_groups restated on the forest text, and the
union of per-group results."""
import numpy as np


def ferns_of(text):
    """[(fern header tokens, [test line tokens])] in file order."""
    tok = text.split()
    n = int(tok[0])
    i, ferns = 1, []
    for _ in range(n):
        fid, scale, nt = tok[i], tok[i + 1], int(tok[i + 2])
        i += 3
        tests = [tok[i + 6 * j:i + 6 * j + 6] for j in range(nt)]
        i += 6 * nt
        ferns.append(((fid, scale), tests))
    return ferns


def group_texts(text, limit=32):
    """One forest text per group: ferns packed greedily into groups of <= limit tests, a longer fern cut into chunks."""
    groups, is_open = [], False
    for head, tests in ferns_of(text):
        if len(tests) > limit:
            for k in range(0, len(tests), limit):
                groups.append([(head, tests[k:k + limit])])
            is_open = False
        elif is_open and sum(len(t) for _, t in groups[-1]) + len(tests) <= limit:
            groups[-1].append((head, tests))
        elif tests or not is_open:
            groups.append([(head, tests)])
            is_open = True
    if not groups:
        groups = [[]]
    out = []
    for g in groups:
        lines = [str(len(g))]
        for (fid, scale), tests in g:
            lines.append("%s %s %d" % (fid, scale, len(tests)))
            lines += [" ".join(t) for t in tests]
        out.append("\n".join(lines) + "\n")
    return out


PLANE_FIRST = (0, 8, 9, 17, 25)              # the first test slot of each byte plane of the SSE hash (k_hash_body.h)
TAU_VALUES = (-127, -20, -1, 1, 20, 127)
TAU_RULES = ("zero", "nonzero", "plane_first", "plane_rest", "alternating")


def fern_split(T, ferns):
    """T tests over 1 fern, 2 ferns or one fern per test ("each"): the reference numbers test slots across ferns."""
    if ferns == "each":
        return [1] * T
    return [T] if ferns == 1 else [(T + 1) // 2, T // 2]


def forest_text(fern_sizes, seed=0, tau=True, scales="l", m128_last=False):
    """A forest of ferns with the given test counts (offsets inside the 27x27 patch).
    tau: True draws every tau from -20 .. 20, False writes 0, and a name of TAU_RULES places the zeros by the test's slot
    (its index over all ferns): "zero" everywhere, "nonzero" nowhere, "plane_first" everywhere but on PLANE_FIRST,
    "plane_rest" on PLANE_FIRST only, "alternating" on the odd slots; the other slots cycle through TAU_VALUES.
    scales: the ferns' scale letters ("s", "m", "l"), cycled.  m128_last: the last test that is kept (slot 31 at most) gets
    a tau of -128."""
    assert tau in (True, False) or tau in TAU_RULES
    rng = np.random.default_rng(seed)
    total = sum(fern_sizes)
    lines = [str(len(fern_sizes))]
    slot = 0
    for f, n in enumerate(fern_sizes):
        lines.append("%d %s %d" % (f, scales[f % len(scales)], n))
        for lvl in range(n):
            ix, iy, jx, jy = rng.integers(-13, 14, 4)
            if tau is True:
                t = int(rng.integers(-20, 21))
            elif tau is False or tau == "zero":
                t = 0
            else:
                is_zero = {"nonzero": False, "plane_first": slot not in PLANE_FIRST, "plane_rest": slot in PLANE_FIRST,
                           "alternating": slot % 2 == 1}[tau]
                t = 0 if is_zero else TAU_VALUES[(slot + seed) % len(TAU_VALUES)]
            if m128_last and slot == min(total, 32) - 1:
                t = -128
            lines.append("%d %d %d %d %d %d" % (lvl, ix, iy, jx, jy, t))
            slot += 1
    return "\n".join(lines) + "\n"


def union(lists, fields):
    """Group 0's records, then every later group's records not equal to one already emitted (compared on `fields`)."""
    seen, keep = set(), []
    for lst in lists:
        for r in lst:
            k = tuple(r[f].item() for f in fields)
            if k not in seen:
                seen.add(k)
                keep.append(r)
    if not keep:
        return lists[0][:0].copy()
    return np.array(keep, dtype=lists[0].dtype)
