"""The scratch contract on the CPU: the case table of tests/workspace_cases.py against include/uoc_hip.h, and the guarded
buffer of tests/scratch_guard.py on CPU tensors.  The device half is tests/test_workspace_contract_gpu.py."""
import re

import pytest
import torch

from tests import scratch_guard as SG
from tests import workspace_cases as WC
from tests.test_native_abi import header_prototypes, header_text
from unseenobjectclustering_amd import _native

SCRATCH_NAMES = {"d_ws", "d_state", "d_mem"}


def header_parameters():
    """{entry: [parameter names]} of every function the header declares: test_native_abi's parser, keeping the names."""
    out = {}
    for _, name, args in re.findall(r"^([A-Za-z_][\w \*]*?)\b(uoc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M):
        out[name] = [] if args.strip() == "void" else [re.search(r"(\w+)$", a.strip()).group(1) for a in args.split(",")]
    return out


def uncovered(cases, exempt):
    """What the table is missing or has too much of, as messages."""
    params = header_parameters()
    takes = {name for name, names in params.items() if SCRATCH_NAMES & set(names)}
    bad = [f"{name}: takes caller scratch or state and has neither a case nor an exemption" for name in sorted(takes - set(cases) - set(exempt))]
    bad += [f"{name}: a case for an entry without d_ws, d_state or d_mem" for name in sorted(set(cases) - takes)]
    bad += [f"{name}: exempt, but the header declares no such entry" for name in sorted(set(exempt) - set(params))]
    bad += [f"{name}: both a case and an exemption" for name in sorted(set(cases) & set(exempt))]
    return bad


def test_every_entry_with_scratch_or_state_has_a_case():
    params = header_parameters()
    assert list(params) == [p[0] for p in header_prototypes()] and len(params) >= 87         # the same declarations, none lost
    assert all(len(names) == len(p[2]) for names, p in zip(params.values(), header_prototypes()))
    assert params["uoc_scene_step"].count("d_mem") == 1 and "d_state" in params["uoc_track_reset"] and "d_ws" in params["uoc_grasp"]
    assert uncovered(WC.CASES, WC.EXEMPT) == []
    assert all(isinstance(reason, str) and reason for reason in WC.EXEMPT.values())


@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_deleting_a_case_is_noticed(name):
    rest = {k: v for k, v in WC.CASES.items() if k != name}
    bad = uncovered(rest, WC.EXEMPT)
    assert len(bad) == 1 and bad[0].startswith(name + ":"), bad


def test_the_table_check_reports_what_does_not_belong():
    assert any(m.startswith("uoc_version:") for m in uncovered({**WC.CASES, "uoc_version": None}, WC.EXEMPT))
    assert any(m.startswith("uoc_nothing:") for m in uncovered(WC.CASES, {**WC.EXEMPT, "uoc_nothing": "x"}))
    assert any(m.startswith("uoc_grasp:") for m in uncovered(WC.CASES, {**WC.EXEMPT, "uoc_grasp": "x"}))


def test_every_case_is_complete():
    for name, case in WC.CASES.items():
        assert case.kind in ("scratch", "signature", "state") and case.align in (16, 256), name
        if case.kind == "state":
            assert name in WC.STATE_STAGES and name.endswith("_reset"), name
        else:
            assert case.shapes and callable(case.run) and callable(case.check), name
    assert set(WC.STATE_STAGES) == {n for n, c in WC.CASES.items() if c.kind == "state"}


# ---- the guarded buffer ---------------------------------------------------------------------------------------------------
def test_canary_differs_from_every_fill():
    pattern = set(SG.canary(0, 4 * SG.CANARY_PERIOD, "cpu").tolist())
    assert len(pattern) == SG.CANARY_PERIOD and not pattern & set(SG.FILLS) and SG.FILLS == (0x00, 0xFF, 0x55)


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("nbytes", [1, 100, 4096, 65537])
@pytest.mark.parametrize("fill", SG.FILLS)
def test_view_has_the_length_the_residue_and_the_fill(nbytes, fill, offset):
    g = SG.guarded("cpu", nbytes, fill, offset)
    assert g.view.dtype == torch.uint8 and g.view.numel() == nbytes and g.view.data_ptr() % 256 == offset == g.address % 256
    assert bool((g.view == fill).all())
    assert g.start >= SG.GUARD and g.buf.numel() - g.end >= SG.GUARD                      # at least 4096 canary bytes either side
    assert g.view.data_ptr() == g.buf.data_ptr() + g.start and g.view.untyped_storage().data_ptr() == g.buf.untyped_storage().data_ptr()
    g.check()


def test_a_larger_alignment_than_the_allocators():
    g = SG.guarded("cpu", 1000, 0x55, 256, align=512)
    assert g.address % 512 == 256
    g.check()


@pytest.mark.parametrize("distance", [1, 2, 4096])
@pytest.mark.parametrize("side", ["before", "after"])
def test_a_write_outside_the_view_is_reported_with_its_distance(side, distance):
    g = SG.guarded("cpu", 300, 0xFF, 16, name="fake_entry_bytes")

    def fake_entry(ws, ws_bytes):                # writes one byte `distance` bytes outside [ws, ws + ws_bytes)
        whole = torch.empty(0, dtype=torch.uint8).set_(ws.untyped_storage())
        at = ws.storage_offset() + (-distance if side == "before" else ws_bytes - 1 + distance)
        whole[at] = 0

    fake_entry(g.view, g.view.numel())
    assert g.damage()[:2] == (side, distance)
    with pytest.raises(SG.GuardError, match=rf"fake_entry_bytes: canary changed {distance} byte\(s\) {side} the 300-byte view"):
        g.check()


def test_the_nearest_of_two_writes_in_front_is_not_the_first_in_memory():
    """`first changed byte`: in address order, so in front of the view it is the one farthest from it."""
    g = SG.guarded("cpu", 64, 0, 0)
    g.buf[g.start - 1] = 0
    g.buf[g.start - 9] = 0
    assert g.damage()[:2] == ("before", 9)


def test_writes_inside_the_view_are_not_reported():
    g = SG.guarded("cpu", 300, 0x55, 16)
    g.view[0], g.view[299] = 0, 0xA0
    g.view[100:200] = 0xFF
    g.check()
    assert g.damage() is None


def test_a_canary_byte_rewritten_with_its_own_value_is_no_damage_but_any_other_value_is():
    g = SG.guarded("cpu", 32, 0, 0)
    i = g.end + 5
    g.buf[i] = SG.CANARY_BASE + i % SG.CANARY_PERIOD
    g.check()
    for fill in SG.FILLS:
        g.buf[i] = fill
        assert g.damage()[:2] == ("after", 6)


def test_the_patch_hands_out_exact_guarded_views_records_them_and_restores_the_function():
    real = _native.workspace
    lib = _native.lib()
    with SG.guard_workspaces(0x55, 16) as rec:
        assert _native.workspace is not real
        a = _native.workspace("uoc_relations_workspace_bytes", "cpu", 2, 37, 53, who="t", hint="h")
        b = _native.workspace("uoc_track_workspace_bytes", "cpu", 2, who="t", hint="h", floor=16)
        z = _native.workspace("uoc_signature_workspace_bytes", "cpu", 2, who="t", hint="h", zero=True)
        with pytest.raises(_native.NativeError, match="t: bad shape h"):
            _native.workspace("uoc_relations_workspace_bytes", "cpu", 0, 37, 53, who="t", hint="h")
    assert _native.workspace is real
    assert a.numel() == lib.uoc_relations_workspace_bytes(2, 37, 53) and b.numel() == lib.uoc_track_workspace_bytes(2)
    assert z.numel() == lib.uoc_signature_workspace_bytes(2) and not z.any() and bool((a == 0x55).all()) and bool((b == 0x55).all())
    assert rec.table() == [("uoc_relations_workspace_bytes", a.numel(), a.data_ptr()), ("uoc_track_workspace_bytes", b.numel(), b.data_ptr()),
                           ("uoc_signature_workspace_bytes", z.numel(), z.data_ptr())]
    assert all(addr % 256 == 16 for _, _, addr in rec.table())


def test_the_patch_verifies_every_canary_on_exit_and_restores_the_function_when_it_fails():
    real = _native.workspace
    with pytest.raises(SG.GuardError, match="uoc_track_workspace_bytes: canary changed 1 byte"):
        with SG.guard_workspaces(0xFF) as rec:
            _native.workspace("uoc_relations_workspace_bytes", "cpu", 1, 8, 8, who="t", hint="h")
            _native.workspace("uoc_track_workspace_bytes", "cpu", 1, who="t", hint="h")
            g = rec.items[1]
            g.buf[g.end] = 0x55
    assert _native.workspace is real


def test_a_state_hand_out_takes_the_state_fill():
    with SG.guard_workspaces(0x55, state_fill=0xFF) as rec:
        s = _native.workspace("uoc_ident_state_bytes", "cpu", 2, who="t", hint="h")
        w = _native.workspace("uoc_ident_workspace_bytes", "cpu", 2, who="t", hint="h")
    assert bool((s == 0xFF).all()) and bool((w == 0x55).all()) and rec.names() == ["uoc_ident_state_bytes", "uoc_ident_workspace_bytes"]


# ---- the allocations routed through _native.workspace return what they returned before --------------------------------------
def test_routed_allocations_keep_their_sizes():
    lib = _native.lib()
    B, H, W = 2, 37, 53
    ws = _native.workspace("uoc_objects_workspace_bytes", "cpu", B, H, W, who="t", hint="h", floor=1)
    assert ws.dtype == torch.uint8 and ws.numel() == max(lib.uoc_objects_workspace_bytes(B, H, W), 1) > 1
    assert _native.workspace("uoc_objects_workspace_bytes", "cpu", 0, H, W, who="t", hint="h", floor=1).numel() == 1     # the entry reports it
    assert _native.workspace("uoc_ms_confidence_workspace_bytes", "cpu", B, 1961, 100, 2, who="t", hint="h", floor=16).numel() == \
        max(lib.uoc_ms_confidence_workspace_bytes(B, 1961, 100, 2), 16)
    assert _native.workspace("uoc_track_workspace_bytes", "cpu", B, who="t", hint="h", floor=16).numel() == max(lib.uoc_track_workspace_bytes(B), 16)
    acc = _native.workspace("uoc_signature_workspace_bytes", "cpu", B, who="t", hint="h", zero=True)
    assert acc.numel() == lib.uoc_signature_workspace_bytes(B) and not acc.any()
    from unseenobjectclustering_amd import identity
    assert lib.uoc_signature_workspace_bytes(3) == 3 * identity._ACC_BYTES
