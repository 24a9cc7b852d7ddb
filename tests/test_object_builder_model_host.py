"""The object builder's edge cases without a GPU (tests/golden/object_builder_edges.npz, written
by make_golden_object_builder_edges.py from the reference's own merge and mean_descriptors):

* the regenerated inputs have the recorded digests, and the oracle and the device=None path give
  the reference's bits on clusters of 63 .. 200 members and on wide-exponent descriptor banks;
* the dim = 1 statement: there the reference sums pairwise, device=None follows it, and the
  sequential oracle (what the kernel computes) differs;
* the pruned neighbour search the n = 65536 GPU test relies on equals the oracle's full walk;
* the sensitivity table: each wrong variant of a kernel step, written in numpy, differs from the
  oracle on the new inputs, and -- where marked -- equals it on the first suite's inputs, which
  is why those could not have caught it."""
import functools

import numpy as np
import pytest

import object_builder_cases as C
import object_builder_oracle as O
from conftest import golden
from onepose_amd import object_builder as ob


def same(a, ref):
    a, ref = np.asarray(a), np.asarray(ref)
    return a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes()


@pytest.fixture(scope="module")
def g():
    return golden("object_builder_edges")


@functools.lru_cache(maxsize=None)
def lifted(n3, dim, wide=True):
    args = C.lift_inputs(n3, dim, wide)
    return args, O.lift(*args, dim)


# ------------------------------------------------------------------ digests
@pytest.mark.parametrize("name", list(C.LONG_MERGE_CASES))
def test_long_clusters_equal_the_reference(g, name):
    xyz, ids, thr, groups = C.long_merge_case(name)
    assert C.sha(xyz, ids) == str(g[f"merge_{name}_sha"]), "synthetic inputs changed"
    for fn in (lambda: ob.merge(xyz, ids, thr), lambda: O.merge(xyz, ids, thr)):
        pts, ret = fn()
        lens, flat = C.flatten_clusters(ret)
        assert same(pts, g[f"merge_{name}_points"])
        assert same(lens, g[f"merge_{name}_lens"]) and same(flat, g[f"merge_{name}_ids"])
    lens = g[f"merge_{name}_lens"]
    for size in C.LONG_SIZES:
        assert (lens == size).sum() == (2 if size == 65 else 1)
    kept = set(g[f"merge_{name}_ids"].tolist())
    skip = groups["skip"][0]
    assert all(ids[r] in kept for r in skip[:65]) and ids[skip[65]] not in kept
    rs, cols = O.radius_neighbours(xyz, thr)
    assert rs[skip[64] + 1] - rs[skip[64]] == 66       # the skipped row is longer than a wave


@pytest.mark.parametrize("n3,dim", C.LIFT_ALL)
def test_wide_lifting_equals_the_reference(g, n3, dim):
    args, (ss, collected, mean64, mean32) = lifted(n3, dim)
    assert C.sha(*args) == str(g[f"lift_{n3}_{dim}_in_sha"]), "synthetic inputs changed"
    ncols, seg = args[2], args[5]
    assert len(seg) == n3 and len(ncols) == 1500 and ncols.min() == 1 and ncols.max() == 39
    assert len(np.setdiff1d(np.arange(1500), args[3])) >= C.LIFT_UNUSED
    assert seg[3] == 519 and seg[5] == 1300 and seg[-1] == 65 and ss[5] < 1024 < ss[6]
    if dim >= 2:
        assert C.sha(mean64) == str(g[f"lift_{n3}_{dim}_ref_sha"])
    else:       # numpy sums a contiguous [k, 1] block pairwise: the reference is not sequential
        assert C.sha(mean64) == str(g[f"lift_{n3}_{dim}_oracle_sha"])
        assert C.sha(mean64) != str(g[f"lift_{n3}_{dim}_ref_sha"])


@pytest.mark.parametrize("n3,dim", [(2500, 256), (1025, 2), (1025, 1), (2500, 1)])
def test_host_path_lifting_equals_the_reference(g, n3, dim):
    """device=None takes the reference's route (np.mean on a [k, dim] block), at dim 1 too."""
    (bank, off, ncols, blk, feat, seg), (_, collected, mean64, _) = lifted(n3, dim)
    col, m64, m32 = ob.lift_descriptors(C.lift_blocks(bank, off, ncols, dim), blk, feat, seg)
    assert same(col, collected)
    assert C.sha(m64) == str(g[f"lift_{n3}_{dim}_ref_sha"]) and same(m32, m64.astype(np.float32))
    assert same(m64, mean64) == (dim >= 2)


# ------------------------------------------------------------------ the pruned search
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pruned_search_equals_the_oracle(dtype):
    cases = [(C.cloud_points(4096, dtype), C.THR), C.special_cloud(dtype)]
    if dtype == np.float64:
        cases += [C.underflow_case(), (C.sq_separator(), C.THR32)]
    for x, thr in cases:
        rs, cols = O.radius_neighbours(x, thr)
        prs, pcols = C.pruned_neighbours(x, thr)
        assert same(prs, rs) and same(pcols, cols)


def test_special_values_as_the_contract_reads():
    for dtype in (np.float32, np.float64):
        x, thr = C.special_cloud(dtype)
        rs, cols = O.radius_neighbours(x, thr)
        sizes = np.diff(rs)
        assert sizes[60:63].tolist() == [1, 1, 1]      # NaN; inf and inf: inf - inf is NaN
        assert sizes[63:65].tolist() == [2, 2]         # the planted pair
        if dtype == np.float64:
            assert sizes[-2:].tolist() == [1, 1]       # 1e200 apart: the square overflows
    x, thr = C.underflow_case()
    rs, cols = O.radius_neighbours(x, thr)
    assert cols[rs[0]:rs[1]].tolist() == [0, 1, 4] and np.diff(rs).tolist() == [3, 3, 1, 1, 3]


def test_big_cloud_is_what_the_gpu_test_needs():
    x, pairs, triple = C.big_cloud()
    assert x.shape == (65536, 3) and x.dtype == np.float32
    assert triple == (1, 65534, 65535) and pairs[0] == (0, 40000)
    xd = x.astype(np.float64)
    for a, b in pairs + [(triple[0], triple[1]), (triple[0], triple[2]), (triple[1], triple[2])]:
        assert np.sqrt(((xd[a] - xd[b]) ** 2).sum()) < 0.9 * C.THR


# ------------------------------------------------------------------ the sensitivity table
def greedy(x, row_start, cols, mean=C.mean_in_order, seen_entries=None, trust_alone=False):
    """O.merge_greedy with switches for the wrong variants: ``mean`` (x, rows) -> position,
    ``seen_entries`` the number of a row's entries tested against the recorded set,
    ``trust_alone`` a row holding its own point alone starts a cluster without that test."""
    n = x.shape[0]
    recorded = np.zeros(n, dtype=bool)
    cluster_of = np.full(n, -1, dtype=np.int32)
    member_start, members, means = [0], [], []
    for j in range(n):
        nb = cols[row_start[j]:row_start[j + 1]]
        alone = len(nb) == 1 and nb[0] == j
        if not (trust_alone and alone) and recorded[nb[:seen_entries]].any():
            continue
        means.append(mean(x, [int(i) for i in nb]))
        recorded[nb] = True
        cluster_of[nb] = len(means) - 1
        members.extend(int(i) for i in nb)
        member_start.append(len(members))
    return (cluster_of, np.asarray(member_start, dtype=np.int32),
            np.asarray(members, dtype=np.int32), np.asarray(means, dtype=np.float64).reshape(-1, 3))


def equal_merge(a, b):
    return all(same(u, v) for u, v in zip(a, b))


def neighbours(x, thr, how):
    """O.radius_neighbours with the test 'squared' (s < thr * thr) or the arithmetic 'float32'."""
    xd = np.asarray(x).astype(np.float32 if how == "float32" else np.float64)
    n, rows = xd.shape[0], []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            d = xd - xd[j]
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            hit = s < thr * thr if how == "squared" else np.sqrt(s).astype(np.float64) < thr
            hit[j] = True
            rows.append(np.nonzero(hit)[0].astype(np.int32))
    row_start = np.zeros(n + 1, dtype=np.int64)
    row_start[1:] = np.cumsum([len(r) for r in rows])
    return row_start, np.concatenate(rows)


def equal_csr(a, b):
    return same(a[0], b[0]) and same(a[1], b[1])


def filter_without_base(tl, min_track):
    """The compaction's index output when every 1024-chunk starts writing at 0 again."""
    keep = np.asarray(tl) >= min_track
    index = np.full(len(keep), -1, dtype=np.int32)
    for start in range(0, len(keep), 1024):
        k = np.nonzero(keep[start:start + 1024])[0]
        index[:len(k)] = start + k
    return index[:keep.sum()]


def starts_without_carry(seg):
    out = np.zeros(len(seg) + 1, dtype=np.int32)
    for start in range(0, len(seg), 1024):
        c = np.cumsum(seg[start:start + 1024])
        out[start + 1:start + 1 + len(c)] = c
        out[start] = 0
    return out


def test_variant_helpers_are_the_oracle_when_nothing_is_switched():
    x, rs, cols = C.csr_case("lanes", np.float32)
    assert equal_merge(greedy(x, rs, cols), O.merge_greedy(x, rs, cols))
    x, _, thr, _ = C.long_merge_case("long32")
    rs, cols = O.radius_neighbours(x, thr)
    assert equal_merge(greedy(x, rs, cols), O.merge_greedy(x, rs, cols))


@functools.lru_cache(maxsize=None)
def old_cloud():
    x = C.cloud_points(4096, np.float32)
    rs, cols = O.radius_neighbours(x, C.THR)
    return x, rs, cols, O.merge_greedy(x, rs, cols)


@functools.lru_cache(maxsize=None)
def long32():
    x, _, thr, _ = C.long_merge_case("long32")
    rs, cols = O.radius_neighbours(x, thr)
    return x, rs, cols, O.merge_greedy(x, rs, cols)


def test_sensitivity_cluster_mean_by_partial_sums():
    partial = functools.partial(C.mean_in_order, chunk=64)
    x, rs, cols, want = old_cloud()
    assert equal_merge(greedy(x, rs, cols, mean=partial), want)          # old inputs: blind
    x, rs, cols, want = long32()
    got = greedy(x, rs, cols, mean=partial)
    assert same(got[2], want[2]) and not same(got[3], want[3])
    sizes = np.diff(want[1])
    changed = (got[3] != want[3]).any(axis=1)
    assert sorted(sizes[changed]) == [128, 129, 200]     # up to 65 members the variant IS sequential


def test_sensitivity_cluster_mean_reversed():
    x, rs, cols, want = long32()
    got = greedy(x, rs, cols, mean=lambda x, r: C.mean_in_order(x, r[::-1]))
    sizes = np.diff(want[1])
    changed = (got[3] != want[3]).any(axis=1)
    assert changed[sizes >= 63].all() and (sizes >= 63).sum() == 7
    x, rs, cols = C.csr_case("row_order", np.float32)        # the row's order, not ascending order
    want = O.merge_greedy(x, rs, cols)
    assert not same(greedy(x, rs, cols, mean=lambda x, r: C.mean_in_order(x, sorted(r)))[3], want[3])


def test_sensitivity_seen_on_the_first_64_entries():
    x, rs, cols, want = old_cloud()
    assert equal_merge(greedy(x, rs, cols, seen_entries=64), want)       # old inputs: blind
    x, rs, cols, want = long32()
    assert equal_merge(greedy(x, rs, cols, seen_entries=64), want)       # long clusters alone: blind
    for dtype in (np.float32, np.float64):
        x, rs, cols = C.csr_case("seen_at_100", dtype)
        want = O.merge_greedy(x, rs, cols)
        assert want[0][1] == -1 and rs[2] - rs[1] == 130 and cols[rs[1] + 100] == 0
        assert not equal_merge(greedy(x, rs, cols, seen_entries=64), want)


def test_sensitivity_alone_row_taken_as_fresh():
    x, rs, cols, want = old_cloud()
    assert equal_merge(greedy(x, rs, cols, trust_alone=True), want)      # a symmetric CSR: blind
    for name in ("asym_ab", "row_order", "not_self"):
        x, rs, cols = C.csr_case(name, np.float64)
        want = O.merge_greedy(x, rs, cols)
        assert not equal_merge(greedy(x, rs, cols, trust_alone=True), want), name
    x, rs, cols = C.csr_case("asym_ba", np.float64)
    assert O.merge_greedy(x, rs, cols)[0][40] == -1


def test_sensitivity_lifting_scan_without_the_carry():
    seg = C.lift_inputs_old(3)[5]
    assert same(starts_without_carry(seg), O.lift(*C.lift_inputs_old(3), 3)[0])   # n3 = 11: blind
    for n3 in C.LIFT_N3:
        seg = C.lift_structure(n3)[3]
        want = np.concatenate([[0], np.cumsum(seg)]).astype(np.int32)
        assert same(starts_without_carry(seg), want) == (n3 <= 1024)


def test_sensitivity_lifting_mean_order(g):
    args = C.lift_inputs_old(256)
    _, collected, mean64, _ = O.lift(*args, 256)
    for how in ("reversed", "pairwise"):                                   # old bank: blind
        assert same(C.segment_means(collected, args[5], how), mean64)
    assert g["blind_old_case_changed"].tolist() == [0, 0]
    assert g["blind_randn_2500_changed"].tolist() == [0, 0]
    args, (_, collected, mean64, _) = lifted(2500, 256)
    for how, key in (("reversed", "wide_reversed_changed"), ("pairwise", "wide_pairwise_changed")):
        changed = int((C.segment_means(collected, args[5], how) != mean64).any(axis=0).sum())
        assert changed == int(g[key]) >= 2500 // 4


def test_sensitivity_filter_positions_without_base():
    for n in (1, 63, 64, 65, 1000, 1023, 1024):                           # one chunk: blind
        tl = C.filter_pattern(n, "alternate")
        assert same(filter_without_base(tl, 3), O.filter_points(np.zeros((n, 3)), tl, 3, None)[1])
    for n in C.FILTER_N[2:]:
        for pattern in ("all", "first", "last", "alternate"):
            tl = C.filter_pattern(n, pattern)
            want = O.filter_points(np.zeros((n, 3)), tl, 3, None)[1]
            assert not same(filter_without_base(tl, 3), want), (n, pattern)


def test_filter_patterns_keep_what_they_say():
    n = 3073
    kept = {p: np.nonzero(C.filter_pattern(n, p) >= 3)[0] for p in C.FILTER_PATTERNS}
    assert len(kept["all"]) == n and len(kept["none"]) == 0
    assert kept["first"].tolist() == [0, 1024, 2048, 3072]
    assert kept["last"].tolist() == [1023, 2047, 3071, 3072]
    assert np.array_equal(kept["hole"], np.r_[0:1024, 2048:3073])
    assert np.array_equal(kept["alternate"], np.arange(0, n, 2))


def test_sensitivity_distance_compared_squared():
    """`s < thr * thr` against `sqrt(s) < thr`.  At thr = 1e-3 the two agree on every double s
    (the last s below thr * thr already has a root that rounds below thr), so no input at that
    threshold can separate them, the fixtures' edge pairs included; at thr = float32(1e-3) the s
    one ulp below thr * thr has a root that rounds to thr, and C.sq_separator() is a pair with
    exactly that s."""
    t = C.THR * C.THR
    for s in (t, np.nextafter(t, 0.0), np.nextafter(np.nextafter(t, 0.0), 0.0), np.nextafter(t, 1.0)):
        assert (np.sqrt(s) < C.THR) == (s < t)
    for name in C.MERGE_CASES:                                             # old edge pairs: blind
        x, _, thr, _ = C.merge_case(name)
        assert equal_csr(neighbours(x, thr, "squared"), O.radius_neighbours(x, thr)), name
    x = C.sq_separator()
    want = O.radius_neighbours(x, C.THR32)
    assert np.diff(want[0]).tolist() == [1, 1]
    assert np.diff(neighbours(x, C.THR32, "squared")[0]).tolist() == [2, 2]


def test_sensitivity_distance_in_float32():
    """The float64 fixture's edge pairs one ulp below the threshold already separate float32
    arithmetic; no float32 input of the first suite does, and C.f32_separator() (rows 65 and 66
    of the special cloud) is one."""
    x, _, thr, groups = C.merge_case("f64")
    assert not equal_csr(neighbours(x, thr, "float32"), O.radius_neighbours(x, thr))
    g0 = golden("object_builder")
    below = [tuple(p) for p, b in zip(g0["merge_f64_edge_pairs"], g0["merge_f64_edge_below"]) if b]
    rs, cols = neighbours(x, thr, "float32")
    assert below and all(q not in cols[rs[p]:rs[p + 1]] for p, q in below)
    for name in ("f32", "f32e"):                                           # old float32 inputs: blind
        x, _, thr, _ = C.merge_case(name)
        assert equal_csr(neighbours(x, thr, "float32"), O.radius_neighbours(x, thr)), name
    x, thr = C.special_cloud(np.float32)
    assert same(x[65:67], C.f32_separator())
    want, got = O.radius_neighbours(x, thr), neighbours(x, thr, "float32")
    assert (66 in want[1][want[0][65]:want[0][66]]) != (66 in got[1][got[0][65]:got[0][66]])
