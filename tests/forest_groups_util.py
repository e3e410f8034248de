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


def forest_text(fern_sizes, seed=0, tau=True):
    """A forest of ferns with the given test counts (offsets inside the 27x27 patch)."""
    rng = np.random.default_rng(seed)
    lines = [str(len(fern_sizes))]
    for f, n in enumerate(fern_sizes):
        lines.append("%d l %d" % (f, n))
        for lvl in range(n):
            ix, iy, jx, jy = rng.integers(-13, 14, 4)
            t = int(rng.integers(-20, 21)) if tau else 0
            lines.append("%d %d %d %d %d %d" % (lvl, ix, iy, jx, jy, t))
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
