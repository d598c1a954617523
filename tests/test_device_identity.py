"""The classifier of tools/device_identity.py on synthetic assembly lines (nothing is compiled): which pairs of units
count as identical, as identical up to commutative source order, and as different."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("device_identity_mod", os.path.join(ROOT, "tools", "device_identity.py"))
di = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(di)

HEAD = ["\ts_waitcnt vmcnt(0)", "\tv_mul_f64 v[6:7], v[2:3], v[2:3]"]
TAIL = ["\tv_sqrt_f64_e32 v[8:9], v[0:1]", "\ts_endpgm"]


def unit(line):
    return HEAD + [line] + TAIL


def test_identical_pair():
    a = unit("\tv_add_f64 v[0:1], v[2:3], v[4:5]")
    assert di.classify(a, list(a)) == ("identical", None)


def test_add_with_sources_exchanged_is_accepted():
    cls, detail = di.classify(unit("\tv_add_f64 v[0:1], v[2:3], v[4:5]"), unit("\tv_add_f64 v[0:1], v[4:5], v[2:3]"))
    assert cls == "commutative" and detail == {"v_add_f64": 1}
    assert di.commutative_swap("\tv_max_f32_e32 v1, s2, v3", "\tv_max_f32_e32 v1, v3, s2")


def test_sub_with_sources_exchanged_is_different():
    cls, detail = di.classify(unit("\tv_sub_f64 v[0:1], v[2:3], v[4:5]"), unit("\tv_sub_f64 v[0:1], v[4:5], v[2:3]"))
    assert cls == "different" and detail[0][0] == len(HEAD) + 1


def test_add_with_a_neg_on_one_source_is_different():
    assert di.classify(unit("\tv_add_f64 v[0:1], -v[2:3], v[4:5]"), unit("\tv_add_f64 v[0:1], v[4:5], -v[2:3]"))[0] == "different"
    assert di.classify(unit("\tv_add_f64 v[0:1], v[2:3], v[4:5]"), unit("\tv_add_f64 v[0:1], v[4:5], -v[2:3]"))[0] == "different"
    assert not di.commutative_swap("\tv_add_f64 v[0:1], |v[2:3]|, v[4:5]", "\tv_add_f64 v[0:1], v[4:5], |v[2:3]|")
    assert not di.commutative_swap("\tv_add_f32_dpp v0, v1, v2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf",
                                   "\tv_add_f32_dpp v0, v2, v1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")


def test_changed_destination_is_different():
    assert di.classify(unit("\tv_add_f64 v[0:1], v[2:3], v[4:5]"), unit("\tv_add_f64 v[6:7], v[4:5], v[2:3]"))[0] == "different"
    assert di.classify(unit("\tv_add_f64 v[0:1], v[2:3], v[4:5]"), unit("\tv_add_f64 v[6:7], v[2:3], v[4:5]"))[0] == "different"


def test_one_exchange_does_not_excuse_another_difference_or_length():
    a = unit("\tv_add_f64 v[0:1], v[2:3], v[4:5]")
    b = unit("\tv_add_f64 v[0:1], v[4:5], v[2:3]")
    assert di.classify(a, b[:-1] + ["\ts_nop 0"])[0] == "different"
    assert di.classify(a, b + ["\ts_nop 0"])[0] == "different"
    # three sources, or a carry destination, are not the two-source form
    assert not di.commutative_swap("\tv_add_co_u32_e32 v0, vcc, v1, v2", "\tv_add_co_u32_e32 v0, vcc, v2, v1")
    assert not di.commutative_swap("\tv_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]", "\tv_fma_f64 v[0:1], v[4:5], v[2:3], v[6:7]")
