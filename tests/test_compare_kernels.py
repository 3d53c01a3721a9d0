"""The parser of tools/compare_kernels.py on synthetic assembly (no compiler needed)."""
import importlib.util
import os

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "compare_kernels.py")
_spec = importlib.util.spec_from_file_location("compare_kernels", _PATH)
ck = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ck)


def _function(name, ordinal, body="v_add_f32_e32 v0, v0, v1", vgprs=13, kernel=True):
    """One function as the compiler prints it, the `ordinal`-th of its file."""
    descriptor = f"""\
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {name}
		.amdhsa_group_segment_fixed_size 4160
		.amdhsa_next_free_vgpr {vgprs}
		.amdhsa_next_free_sgpr 20
	.end_amdhsa_kernel
	.text
""" if kernel else ""
    return f"""\
	.protected	{name}                  ; -- Begin function {name}
	.globl	{name}
	.p2align	8
	.type	{name},@function
{name}:                                 ; @{name}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB{ordinal}_1:                        ; %loop
                                        ; =>This Inner Loop Header: Depth=1
	{body}
	s_cbranch_scc1 .LBB{ordinal}_1
; %bb.2:                                ;   in Loop: Header=BB{ordinal}_1 Depth=1
	s_endpgm
{descriptor}.Lfunc_end{ordinal}:
	.size	{name}, .Lfunc_end{ordinal}-{name}
                                        ; -- End function
	.set {name}.num_vgpr, {vgprs}
	.set {name}.private_seg_size, 0
"""


def _compare(old, new):
    return ck.compare(ck.parse(old), ck.parse(new))


NOTHING = {"only_old": [], "only_new": [], "code": [], "descriptor": []}


def test_parse_splits_functions_and_descriptors():
    parsed = ck.parse(_function("kern_a", 0) + _function("helper", 1, kernel=False))
    assert sorted(parsed) == ["helper", "kern_a"]
    code, desc = parsed["kern_a"]
    assert "v_add_f32_e32 v0, v0, v1" in code and "s_cbranch_scc1 .LBB_1" in code
    assert not any(";" in line or ".amdhsa" in line for line in code)
    assert ".amdhsa_next_free_vgpr 13" in desc and ".set num_vgpr 13" in desc
    assert ck.is_kernel(parsed["kern_a"]) and not ck.is_kernel(parsed["helper"])


def test_swapped_order_and_renumbered_labels_compare_equal():
    old = _function("kern_a", 0) + _function("kern_b", 1, body="v_mul_f32_e32 v0, v0, v1")
    new = _function("kern_b", 7, body="v_mul_f32_e32 v0, v0, v1") + _function("kern_a", 8)
    assert old != new
    assert _compare(old, new) == NOTHING


def test_changed_instruction_compares_different():
    old = _function("kern_a", 0) + _function("kern_b", 1)
    new = _function("kern_a", 0) + _function("kern_b", 1, body="v_add_f32_e32 v0, v0, v2")
    assert _compare(old, new) == dict(NOTHING, code=["kern_b"])


def test_changed_vgpr_count_compares_different():
    old = _function("kern_a", 0) + _function("kern_b", 1)
    new = old.replace(".amdhsa_next_free_vgpr 13", ".amdhsa_next_free_vgpr 14", 1)
    assert new != old
    assert _compare(old, new) == dict(NOTHING, descriptor=["kern_a"])


def test_missing_function_is_reported():
    both = _function("kern_a", 0) + _function("kern_b", 1)
    one = _function("kern_b", 0)
    assert _compare(both, one) == dict(NOTHING, only_old=["kern_a"])
    assert _compare(one, both) == dict(NOTHING, only_new=["kern_a"])
