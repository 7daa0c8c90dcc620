"""The workspace-size table of test_trainer_ws_bytes_unchanged (no tests here).

Each case is a trainer configuration and the hop sizes of one step, (n_dst,
n_pos, n_src, n_nbr) per hop from the roots down; WS_BYTES[i] is what
gs_trainer_ws_bytes returned for case i on a build of the commit before
run_step was split into stages (a48b49d), so the numbers pin the workspace
carve: its order and every size expression.
"""
FEAT_DIM = 24

_B4 = [(4, 9, 11, 9), (11, 30, 37, 30), (37, 90, 101, 90)]
_B97 = [(97, 700, 611, 700), (611, 5000, 3203, 5000), (3203, 20000, 9001, 20000)]

# (layers, gcn, agg, bf16 features, classes, hidden, hops)
WS_CASES = [
    (1, False, "MEAN", False, 7, 32, _B4),
    (1, True, "MAX", True, 16, 128, _B97),
    (1, False, "MAX", False, 40, 128, _B97),
    (2, False, "MEAN", False, 16, 128, _B97),
    (2, False, "MAX", False, 7, 128, _B4),
    (2, False, "MEAN", True, 40, 128, _B97),
    (2, True, "MEAN", False, 16, 32, _B97),
    (2, True, "MAX", True, 40, 32, _B4),
    (2, False, "MAX", True, 16, 32, _B97),
    (2, False, "MEAN", False, 40, 32, _B4),
    (3, False, "MEAN", False, 7, 128, _B97),
    (3, False, "MAX", True, 40, 32, _B4),
    (3, True, "MEAN", True, 16, 128, _B4),
    (3, True, "MAX", False, 40, 128, _B97),
]

WS_BYTES = [2816, 311040, 625408, 1698816, 36608, 1979136, 434048, 13952, 454016, 14464, 7767296, 31360, 90368,
            7718400]


def hop_sizes(case):
    """The case's flat int64 hop_sizes argument, as a list."""
    layers, hops = case[0], case[6]
    return [v for hop in hops[:layers] for v in hop]
