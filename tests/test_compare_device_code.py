"""scripts/compare_device_code.py on made-up disassembly: what two links of the same code may differ in (addresses, the
pc-relative distance to a constant table, the code object a function is in) is set aside, anything else is a difference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PARENT = ["""
lib.so.1.hipv4-amdgcn-amd-amdhsa--gfx950:	file format elf64-amdgpu

Disassembly of section .text:

0000000000001900 <kernel_a>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001900: C0060002 00000000
	s_getpc_b64 s[2:3]                                         // 000000001908: BE821C00
	s_add_u32 s2, s2, 0xfffe74ec                               // 00000000190C: 8002FF02 FFFE74EC
	s_addc_u32 s3, s3, -1                                      // 000000001914: 8203C103
	s_add_u32 s70, s2, s0                                      // 000000001918: 80460002
	s_cbranch_scc0 314                                         // 00000000191C: BF84013A <kernel_a+0x508>
	s_endpgm                                                   // 000000001920: BF810000
		...

0000000000001a00 <kernel_b>:
	v_add_f32_e32 v1, v2, v3                                   // 000000001A00: 02020702
	s_endpgm                                                   // 000000001A04: BF810000
"""]


def _this(b_body="v_add_f32_e32 v1, v2, v3", with_b=True):
    # kernel_b first and in a code object of its own, kernel_a elsewhere at another address with its table somewhere else
    a = """
Disassembly of section .text:

0000000000004200 <kernel_a>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000004200: C0060002 00000000
	s_getpc_b64 s[2:3]                                         // 000000004208: BE821C00
	s_add_u32 s2, s2, 0xfffd5be4                               // 00000000420C: 8002FF02 FFFD5BE4
	s_addc_u32 s3, s3, -1                                      // 000000004214: 8203C103
	s_add_u32 s70, s2, s0                                      // 000000004218: 80460002
	s_cbranch_scc0 314                                         // 00000000421C: BF84013A <kernel_a+0x508>
	s_endpgm                                                   // 000000004220: BF810000
"""
    b = f"""
0000000000000100 <kernel_b>:
	{b_body}                                   // 000000000100: 02020702
	s_endpgm                                                   // 000000000104: BF810000
"""
    return [b, a] if with_b else [a]


def test_identical_up_to_addresses_tables_and_code_object():
    import compare_device_code as c

    assert c.compare(PARENT, _this()) == (["kernel_a", "kernel_b"], [], [], [])


def test_one_changed_operand_is_different():
    import compare_device_code as c

    assert c.compare(PARENT, _this("v_add_f32_e32 v1, v2, v4")) == (["kernel_a"], ["kernel_b"], [], [])
    # ... and so is another branch distance, or an s_add_u32 literal that is no table address
    moved = [PARENT[0].replace("s_cbranch_scc0 314", "s_cbranch_scc0 315")]
    assert c.compare(PARENT, moved)[1] == ["kernel_a"]
    literal = [PARENT[0].replace("s_add_u32 s70, s2, s0", "s_add_u32 s70, s70, 0x10")]
    assert c.compare(literal, [literal[0].replace("0x10", "0x20")])[1] == ["kernel_a"]


def test_absent_function_is_missing_and_added_one_is_new():
    import compare_device_code as c

    assert c.compare(PARENT, _this(with_b=False)) == (["kernel_a"], [], ["kernel_b"], [])
    assert c.compare(_this(with_b=False), PARENT) == (["kernel_a"], [], [], ["kernel_b"])
