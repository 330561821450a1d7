"""MaxCut's hub route without a GPU: the new entries of the C ABI, their refusals and workspace sizes, and the helper
the two gates read.  Without the feature this module fails at the first missing entry."""
import ctypes
import re

import torch

from tgp import _native
from tgp import kernels as K

ENTRIES = ["tgp_mchub_assign_round_i32", "tgp_mchub_assign_workspace_bytes", "tgp_mchub_layer_f32",
           "tgp_mchub_workspace_bytes"]
BIG = 1 << 31


def refusals(fn, ok, cases):
    for at, value, want in cases:
        args = list(ok)
        args[at] = value
        assert fn(*args) == want, (at, value)


def test_the_entries_are_declared_size_their_workspaces_and_refuse():
    assert sorted(n for n in _native.SIGNATURES if n.startswith("tgp_mchub_")) == ENTRIES
    header = open(_native.HEADER_PATH).read()
    assert sorted(set(re.findall(r"\b(tgp_mchub_[a-z0-9_]+)\s*\(", header))) == ENTRIES
    lib = _native.lib()
    assert lib.tgp_mchub_workspace_bytes(0, 8) == 0 and lib.tgp_mchub_workspace_bytes(3, 0) == 0
    assert lib.tgp_mchub_workspace_bytes(3, K.maxcut_max_width() + 1) == 0
    got = lib.tgp_mchub_workspace_bytes(3, 5)  # a partial row and a flag per chunk
    assert got >= 3 * 5 * 4 + 3 * 4 and got % 256 == 0
    assert lib.tgp_mchub_assign_workspace_bytes(0, 4) == 0 and lib.tgp_mchub_assign_workspace_bytes(1, -1) == 0
    assert lib.tgp_mchub_assign_workspace_bytes(2, 7) >= 2 * 8 * 4  # H x (K + 1) int32
    assert lib.tgp_mchub_assign_workspace_bytes(3, 1000) >= 3 * 1001 * 4
    buf = ctypes.create_string_buffer(4096 + 2048)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    q = p + 1024  # everything below is refused before any launch
    # an empty plan (or no node) is 0 whatever else is handed over, an unknown act included
    assert lib.tgp_mchub_layer_f32(None, None, None, None, None, 0, 0, None, None, None, None, 4, 4, 8, None, 2.0, 7,
                                   None, None, 0, None, None, 0, None) == 0
    assert lib.tgp_mchub_assign_round_i32(None, None, None, None, None, 0, 0, None, 4, 4, 7, None, None, 0, None) == 0
    # the layer's arguments in the header's order: T = 1, C = 8 needs 512 bytes of workspace
    ok = [p, None, p, p, p, 1, 1, p, p, p, None, 4, 4, 8, None, 2.0, 1, q, None, 0, None, p, 4096, None]
    refusals(lib.tgp_mchub_layer_f32, ok,
             [(0, None, -1), (3, None, -1), (4, None, -1), (8, None, -1), (9, None, -1), (21, None, -1), (21, p + 4, -1),
              (13, 0, -1), (13, 65, -1), (16, 3, -1), (17, p, -1), (17, None, -1), (19, 5, -1), (5, -1, -1),
              (22, 256, -2), (22, 511, -2), (11, BIG, -4), (12, BIG, -4), (5, BIG + 1, -4), (6, BIG + 1, -4)])
    assert b"tgp_mchub_layer_f32" in lib.tgp_last_error()
    # the round's: H = 1, K = 7 needs 256 bytes
    ok = [p, None, p, p, p, 1, 1, p, 4, 4, 7, q, p, 4096, None]
    refusals(lib.tgp_mchub_assign_round_i32, ok,
             [(0, None, -1), (4, None, -1), (7, None, -1), (11, None, -1), (11, p, -1), (12, None, -1), (10, -1, -1),
              (13, 31, -2), (10, 1024, -2), (10, BIG, -4), (8, BIG, -4), (6, BIG + 1, -4)])
    assert b"tgp_mchub_assign_round_i32" in lib.tgp_last_error()


def test_the_gates_read_the_longest_group_one_wave_walks(monkeypatch):
    ptr = torch.tensor([0, 9, 9, 17, 20, 5020], dtype=torch.int32)  # groups of 9, 0, 8, 3 and 5000 entries
    grp = K.AssignIndex(ptr, None, 5020, 5)
    assert grp.hub is None and K.maxcut_one_wave_group(grp) == 5000 and K.maxcut_assign_hub_fits(grp, 1 << 40)
    grp.hub = K.build_hub_plan(grp)  # the 5000 entries of node 4 go to the chunked route
    assert grp.hub.hub_ids.tolist() == [4] and K.maxcut_one_wave_group(grp) == K.HUB_MIN_GROUP == 4096
    small = K.AssignIndex(ptr[:5].clone(), None, 20, 4)
    small.hub = K.build_hub_plan(small, min_group=8, chunk=4)
    assert small.hub.hub_ids.tolist() == [0] and K.maxcut_one_wave_group(small) == 9  # (min with the shipped threshold)
    assert K.MAXCUT_ASSIGN_HUB_WS_BYTES == 64 << 20 and K.maxcut_assign_hub_fits(grp, 7)
    monkeypatch.setattr(K, "MAXCUT_ASSIGN_HUB_WS_BYTES", 31)  # 1 hub x 8 counts x 4 bytes = 32
    assert not K.maxcut_assign_hub_fits(grp, 7) and K.maxcut_assign_hub_fits(grp, 6)
