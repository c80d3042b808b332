"""The placement maps of the float32 step kernels (csrc/include/tde_convnet.h: fwd_slot, bwd_slot) decide which
workgroup id does which (position group, image tile) of the forward and which pooled position of the backward, so
that the workgroups that hand W1 rows, Pt rows and argmax words to each other between the two launches have ids of
one class mod 8 (workgroups are dealt round-robin over the 8 XCDs).  A map that is not a bijection would drop or
repeat a piece of the step: read without a GPU, from the built library's host-side export of the whole map."""
import ctypes as C

from tensorflow_distributed_example_amd import _native as N


def _fwd(groups, tiles):
    out = (C.c_int * (2 * groups * tiles))()
    assert N.hip().tde_convnet_slot_map(0, groups, tiles, out) == groups * tiles
    return [(out[2 * i], out[2 * i + 1]) for i in range(groups * tiles)]


def _bwd(P):
    out = (C.c_int * P)()
    assert N.hip().tde_convnet_slot_map(1, P, 0, out) == P
    return list(out)


class identity_slots:
    def __enter__(self):
        self.prev = N.hip().tde_convnet_f32_identity_slots(1)

    def __exit__(self, *exc):
        N.hip().tde_convnet_f32_identity_slots(self.prev)


def test_fwd_slot_is_a_bijection():
    for groups in range(1, 65):
        for tiles in range(1, 9):
            m = _fwd(groups, tiles)
            assert sorted(m) == [(g, y) for g in range(groups) for y in range(tiles)], (groups, tiles)


def test_bwd_slot_is_a_bijection():
    for P in range(1, 201):
        assert sorted(_bwd(P)) == list(range(P)), P


def test_a_groups_tiles_share_a_class_in_full_runs():
    for groups in range(1, 65):
        for tiles in range(1, 9):
            ids = {}
            for i, (g, y) in enumerate(_fwd(groups, tiles)):
                ids.setdefault(g, []).append(i)
            for g in range(8 * (groups // 8)):
                assert {i % 8 for i in ids[g]} == {g % 8}, (groups, tiles, g)


def test_backward_positions_share_their_groups_class():
    """Positions 4g..4g+3 of every group in a full run of 32 positions: the ids of their backward workgroups are
    congruent to the ids of the group's forward workgroups (mod 8); with any tile count."""
    for P in range(1, 201):
        groups = (P + 3) // 4
        at = {p: i for i, p in enumerate(_bwd(P))}
        for tiles in (1, 4, 5):
            fwd = {}
            for i, (g, y) in enumerate(_fwd(groups, tiles)):
                fwd.setdefault(g, set()).add(i % 8)
            for g in range(8 * (P // 32)):
                assert {at[4 * g + j] % 8 for j in range(4)} == fwd[g] == {g % 8}, (P, tiles, g)


def test_the_last_partial_run_keeps_the_launch_order():
    m = _fwd(43, 4)
    assert m[160:] == [(40 + k % 3, k // 3) for k in range(12)]
    assert _bwd(169)[160:] == list(range(160, 169))
    assert _bwd(169)[:32] == [4 * (i % 8) + i // 8 for i in range(32)]


def test_identity_switch():
    with identity_slots():
        for groups, tiles in [(1, 1), (7, 5), (8, 4), (43, 4), (64, 8)]:
            assert _fwd(groups, tiles) == [(i % groups, i // groups) for i in range(groups * tiles)]
        for P in (1, 25, 32, 169, 200):
            assert _bwd(P) == list(range(P))
    assert _bwd(169)[1] == 4   # back on
    assert N.hip().tde_convnet_slot_map(2, 4, 4, (C.c_int * 32)()) == -1
