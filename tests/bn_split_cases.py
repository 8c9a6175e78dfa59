"""The case table of the BatchNorm split tests: shapes at which a workgroup of the row passes of
csrc/bn_relu_pool.hip (fp32 rows) and csrc/bn_relu_pool_h.hip (bf16 rows) owns SEVERAL samples.

Every pass gives a workgroup one channel and the samples [N*s/S, N*(s+1)/S) of split s.  How many splits a channel gets is
decided on the host (csrc/bn_common.h); four counts matter, and a case states all four:

    S    stat_splits(N, C)          the statistics pass and the fp32 backward's reduce pass (and the partials their
                                    consumers combine: the folded statistics combine, the dx pass's combine)
    Sw   stat_splits(N, C, wide)    the bf16 backward's reduce pass
    S2   stream_splits(C, N)        the streaming passes: pool forward, dx pass (fp32 and bf16)
    Sg   gap_fwd_splits(C, N)       the global-average forward (None where L < 2: the pass refuses an empty pooled row)

The numbers were derived by hand; tests/test_bn_splits_host.py asks the library for each of them (no device needed) and
asserts that the table as a whole reaches every regime of REQUIRED, so a case cannot be dropped or drift silently.
tests/test_gpu_bn_splits.py runs the table on the device.
"""

# (id, (N, C, L), (S, Sw, S2, Sg), the regimes the case exists for as "pass:regime")
CASES = [
    # 3+4 and 2+2+3 samples per workgroup; an average split of 3 rows (one wave idle) and one of 4; even L: 8-byte pairs
    ("ragged_small", (7, 1000, 10), (2, 3, 3, 2), ("reduce:ragged", "wide:ragged", "stream:ragged", "gap:ragged")),
    # average splits of 17 / 18 / 18 rows: a second row-batch trip with clamped rows
    ("gap_two_trips", (53, 1000, 6), (2, 3, 3, 3), ("gap:rows_gt_16", "gap:ragged")),
    # combines of more than 256 partials; 2-or-3 and 1-or-2 samples per split; odd L: an unpooled tail sample
    ("many_partials", (700, 3, 9), (342, 683, 683, 175),
     ("reduce:big_combine", "wide:big_combine", "stream:big_combine", "gap:big_combine", "gap:equal")),
    # four-trip combine; S < N by a few samples; the wide and streaming passes at one sample per workgroup
    ("one_channel", (1100, 1, 5), (1024, 1100, 1100, 275), ("reduce:big_combine", "wide:one", "stream:one", "gap:equal")),
    # one workgroup owns all 27 samples in the reduce passes (three trips); 13 / 14 samples and more than 1024 pairs per
    # split in the streaming passes: a partial second trip; odd L: scalar pair loads
    ("walk_trips_odd", (27, 1024, 173), (1, 2, 2, 2), ("reduce:all_in_one", "reduce:walk", "stream:walk", "gap:walk")),
    # the same with 8-byte pair loads
    ("walk_trips_even", (27, 1024, 172), (1, 2, 2, 2), ("reduce:all_in_one", "reduce:walk", "stream:walk", "gap:walk")),
    # every pass is a single workgroup per channel; the average pass takes rows 0 and 4 in one wave's trip
    ("past_2048_channels", (5, 2100, 8), (1, 1, 1, 1), ("reduce:all_in_one", "wide:all_in_one", "stream:all_in_one",
                                                         "gap:all_in_one")),
    # empty pooled row over multi-sample splits (fp32 passes only)
    ("L1", (9, 600, 1), (2, 4, 4, None), ("reduce:ragged", "stream:ragged")),
    # one pair plus a tail sample per row
    ("L3", (9, 600, 3), (2, 4, 4, 3), ("reduce:ragged", "wide:ragged", "stream:ragged", "gap:equal")),
    # splits of the same size, more than one sample each, in every pass: 4+4, 2+2+2+2, 4+4 rows
    ("equal", (8, 600, 4), (2, 4, 4, 2), ("reduce:equal", "wide:equal", "stream:equal", "gap:equal")),
    # the regime every earlier test ran, kept as the table's baseline: one sample per workgroup, second and third
    # workgroup included (n0 > 0)
    ("one_each", (3, 300, 12), (3, 3, 3, 1), ("reduce:one", "wide:one", "stream:one")),
    # the only way the average pass gets one row per workgroup: cdiv(N, 4) >= N
    ("one_sample", (1, 300, 12), (1, 1, 1, 1), ("gap:one",)),
]

# pass -> which of a case's four counts splits it
COUNT_OF = {"reduce": 0, "wide": 1, "stream": 2, "gap": 3}

# What the table as a whole must reach, pass by pass.  The average pass walks ROWS, four per trip and wave: besides more
# than 1024 pairs in a split (rows longer than its 64 lanes) it has "more than 16 rows in a split".  "walk" is a regime of
# the fp32 kernels only and is NOT required of the bf16 reduce pass: the bf16 kernels walk chunks of 8 elements in trips of
# U * 256 chunks, U in 3..6, so a second trip takes more than 1536 chunks — about 25 M elements at the widths that give a
# split several samples, five times the largest tensor these tests may use.  At the walk_trips shapes a bf16 split holds 308
# chunks (154 in the forward): part of ONE trip, the rest of its slots clamped.  No test runs a second bf16 trip.
_COMMON = {"one", "equal", "ragged", "all_in_one", "big_combine"}
REQUIRED = {"reduce": _COMMON | {"walk"}, "wide": _COMMON, "stream": _COMMON | {"walk"},
            "gap": _COMMON | {"walk", "rows_gt_16"}}


def sizes(N, S):
    """samples per split: [N*s/S, N*(s+1)/S) for s < S"""
    return [N * (s + 1) // S - N * s // S for s in range(S)]


def regimes_of(case):
    """{"pass:regime"} a case reaches, from its shape and its four counts alone.

    one          every split is one sample (what every test before this table ran)
    equal        several splits, all of the same size > 1
    ragged       several splits of different sizes
    all_in_one   one split owns all N > 1 samples
    big_combine  the pass combines more than 256 partials: the S statistics partials in a forward, the S (fp32) or Sw
                 (bf16) reduce partials in a dx pass — one more trip of the 256-strided combine loop
    walk         more than 1024 pooling pairs in a split.  In the fp32 reduce and streaming kernels that is more than one
                 trip of the four-deep flat walk; in the average pass, rows longer than a wave.  "stream:walk" speaks of
                 the fp32 streaming kernels; the bf16 kernels' trips are U * 256 chunks of 8 elements and none of them
                 takes a second one at any shape of the table (see REQUIRED), so "wide" has no such regime.
    rows_gt_16   more than 16 rows in a split of the average pass: a second trip of its four-rows-per-wave loop
    """
    _, (N, C, L), counts, _ = case
    out = set()
    for name, k in COUNT_OF.items():
        S = counts[k]
        if S is None or (name == "wide" and L < 2):
            continue
        sz = sizes(N, S)
        assert sum(sz) == N and min(sz) >= 1
        if max(sz) == 1:
            out.add(name + ":one")
        elif S == 1:
            out.add(name + ":all_in_one")
        elif len(set(sz)) == 1:
            out.add(name + ":equal")
        else:
            out.add(name + ":ragged")
        combined = counts[1] if name == "wide" else counts[0]      # partials the pass (or the dx pass behind it) combines
        if combined > 256:
            out.add(name + ":big_combine")
        if name == "gap" and max(sz) > 16:
            out.add("gap:rows_gt_16")
        if name != "wide" and max(sz) * (L // 2) > 1024:
            out.add(name + ":walk")
    return out


def reached(cases=None):
    """pass -> set of regimes the cases reach"""
    out = {k: set() for k in COUNT_OF}
    for c in CASES if cases is None else cases:
        for tag in regimes_of(c):
            p, r = tag.split(":")
            out[p].add(r)
    return out


def up(n, m):
    return (n + m - 1) // m * m
