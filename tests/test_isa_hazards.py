"""tools/isa_hazards.py: the distance between a vector-ALU write and an MFMA that reads the register.

(a) the scanner on synthetic listings in llvm-objdump's format, one exact verdict each; (b) an end-to-end control: a
fixture kernel with the hazard and one without, compiled here and taken through the same extraction as the library, so
an extraction that silently finds nothing cannot pass; (c) the library as built has no violation, and the scan saw the
kernels it is there for.  Nothing here runs on a GPU or loads the library."""
import os
import subprocess

import pytest

import isa_hazards as ih

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MFMA = "v_mfma_f32_16x16x32_f16"


def listing(*kernels):
    """(symbol, [instruction text | (instruction text, size in bytes)]) -> a listing as llvm-objdump -d prints it."""
    out, addr = ["", "x.co:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""], 0x1000
    for sym, body in kernels:
        addr = (addr + 0xFF) & ~0xFF
        out.append(f"{addr:016x} <{sym}>:")
        for ins in body:
            text, size = ins if isinstance(ins, tuple) else (ins, 8 if ins.startswith(("v_mfma", "v_fma_mix")) else 4)
            out.append(f"\t{text:<58} // {addr:012X}: " + " ".join(["BF800000"] * (size // 4)))
            addr += size
        out.append("")
    return "\n".join(out)


def verdicts(*kernels):
    rep = ih.scan_listing(listing(*kernels))
    return [(v.kernel, v.producer.text.split()[0], v.slot, v.states) for v in rep.violations]


def one(*between, producer="v_cvt_pk_f16_f32 v53, v1, v2", consumer=f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]"):
    return verdicts(("k", ["s_mov_b32 s0, 0", producer, *between, consumer, "s_endpgm"]))


def hit(slot, states, producer="v_cvt_pk_f16_f32"):
    return [("k", producer, slot, states)]


def test_zero_and_one_state_are_flagged():
    assert one() == hit("B", 0)
    assert one("v_add_f32_e32 v9, v8, v7") == hit("B", 1)


def test_s_nop_0_is_one_state_and_s_nop_1_is_two():
    assert one("s_nop 0") == hit("B", 1)
    assert one("s_nop 1") == []
    assert one("s_nop 4") == []


def test_two_unrelated_instructions_are_enough():
    assert one("v_add_f32_e32 v9, v8, v7", "s_add_u32 s3, s3, 1") == []
    assert one("s_nop 0", "s_nop 0") == []


def test_a_wait_alone_is_not_credited():
    assert one("s_waitcnt vmcnt(0)") == hit("B", 1)
    assert one("s_waitcnt vmcnt(0) lgkmcnt(0)") == hit("B", 1)
    assert one("s_waitcnt vmcnt(0)", "s_nop 0") == []


@pytest.mark.parametrize("reg,flagged", [("v49", False), ("v50", True), ("v52", True), ("v53", True), ("v54", False)])
def test_register_inside_and_just_outside_the_consumers_range(reg, flagged):
    # B is v[50:53]; A, C and D lie elsewhere
    got = one(producer=f"v_cvt_pk_f16_f32 {reg}, v1, v2", consumer=f"{MFMA} v[92:95], v[60:63], v[50:53], v[66:69]")
    assert got == (hit("B", 0) if flagged else [])


@pytest.mark.parametrize("dst,flagged", [("v[46:49]", False), ("v[47:50]", True), ("v[50:51]", True), ("v[53:54]", True),
                                         ("v[54:55]", False)])
def test_producer_range_against_the_consumers_range(dst, flagged):
    got = one(producer=f"v_pk_mul_f32 {dst}, v[2:3], v[4:5]", consumer=f"{MFMA} v[92:95], v[60:63], v[50:53], v[66:69]")
    assert got == (hit("B", 0, "v_pk_mul_f32") if flagged else [])


def test_each_operand_slot_and_never_the_destination():
    cons = f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]"
    assert one(producer="v_mov_b32_e32 v55, v1", consumer=cons) == hit("A", 0, "v_mov_b32_e32")
    assert one(producer="v_mov_b32_e32 v50, v1", consumer=cons) == hit("B", 0, "v_mov_b32_e32")
    assert one(producer="v_mov_b32_e32 v69, v1", consumer=cons) == hit("C", 0, "v_mov_b32_e32")
    assert one(producer="v_mov_b32_e32 v93, v1", consumer=cons) == []  # D is written, not read
    # accumulating in place: D = C, the read counts
    assert one(producer="v_mov_b32_e32 v93, v1", consumer=f"{MFMA} v[92:95], v[54:57], v[50:53], v[92:95]") == hit("C", 0, "v_mov_b32_e32")
    # an inline constant as C is no register
    assert one(producer="v_mov_b32_e32 v0, v1", consumer=f"{MFMA} v[92:95], v[54:57], v[50:53], 0") == []


def test_only_vector_alu_destinations_are_producers():
    cons = f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]"
    assert one(producer="v_cmp_gt_f32_e32 vcc, v50, v51", consumer=cons) == []          # writes vcc, reads v50
    assert one(producer="v_readfirstlane_b32 s4, v50", consumer=cons) == []
    assert one(producer="v_add_f32_e32 v9, v50, v51", consumer=cons) == []              # a source is no write
    assert one(producer="s_mov_b32 s50, 0", consumer=cons) == []
    assert one(producer="v_add_co_u32_e32 v51, vcc, v1, v2", consumer=cons) == hit("B", 0, "v_add_co_u32_e32")
    assert one(producer="v_permlane32_swap_b32_e32 v7, v56", consumer=cons) == hit("A", 0, "v_permlane32_swap_b32_e32")


def test_accvgpr_write_into_an_agpr_operand():
    cons = f"{MFMA} a[0:3], v[54:57], v[50:53], a[0:3]"
    assert one(producer="v_accvgpr_write_b32 a2, v9", consumer=cons) == hit("C", 0, "v_accvgpr_write_b32")
    assert one("s_nop 0", producer="v_accvgpr_write_b32 a2, v9", consumer=cons) == hit("C", 1, "v_accvgpr_write_b32")
    assert one("s_nop 1", producer="v_accvgpr_write_b32 a2, v9", consumer=cons) == []
    assert one(producer="v_accvgpr_write_b32 a4, v9", consumer=cons) == []
    assert one(producer="v_mov_b32_e32 v2, v9", consumer=cons) == []                    # v2 is not a2
    assert one(producer="v_accvgpr_write_b32 a55, v9", consumer=f"{MFMA} a[0:3], a[54:57], v[50:53], a[0:3]") == hit("A", 0, "v_accvgpr_write_b32")


def test_accumulate_chains_stay_clean():
    body = ["v_mov_b32_e32 v1, 0", "s_nop 1"]
    body += [f"{MFMA} v[92:95], v[54:57], v[50:53], v[92:95]"] * 4
    body += [f"{MFMA} v[80:83], v[54:57], v[50:53], v[92:95]", f"{MFMA} v[84:87], v[80:83], v[50:53], v[84:87]", "s_endpgm"]
    rep = ih.scan_listing(listing(("k", body)))
    assert rep.violations == [] and rep.mfmas == 6 and rep.producers == 1


def test_producer_before_a_branch_whose_target_starts_with_the_mfma():
    # 0x1000 .. : producer (8 bytes), s_cbranch_scc1 +2 dwords, two fillers, the MFMA
    body = ["v_fma_mixhi_f16 v53, v49, -1.0, v96 op_sel:[1,0,0] op_sel_hi:[1,0,0]", "s_cbranch_scc1 2",
            "v_add_f32_e32 v9, v8, v7", "v_add_f32_e32 v10, v8, v7", f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]", "s_endpgm"]
    rep = ih.scan_listing(listing(("k", body)))
    assert [(v.slot, v.states, [i.mnemonic for i in v.between]) for v in rep.violations] == [("B", 1, ["s_cbranch_scc1"])]
    # the fall-through path alone (three states) is clean
    assert verdicts(("k", body[:1] + ["s_nop 0"] + body[2:])) == []
    # an unconditional branch is followed to its target only: the MFMA behind it is not reached in fall-through
    jump = ["v_mov_b32_e32 v50, v1", "s_branch 2", f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]",
            f"{MFMA} v[92:95], v[50:53], v[60:63], v[66:69]", "s_endpgm"]
    assert verdicts(("k", jump)) == hit("A", 1, "v_mov_b32_e32")
    # a backward branch (the offset printed as an unsigned 16-bit number): the loop head reads what the loop tail wrote
    loop = [f"{MFMA} v[92:95], v[54:57], v[50:53], v[92:95]", "v_add_f32_e32 v9, v8, v7", "v_add_f32_e32 v10, v8, v7",
            "v_mov_b32_e32 v57, v1", "s_cbranch_scc0 65530", "s_endpgm"]
    assert verdicts(("k", loop)) == hit("A", 1, "v_mov_b32_e32")


def test_two_kernels_in_one_listing_the_violation_goes_to_the_right_symbol():
    bad = ["v_mov_b32_e32 v50, v1", "s_nop 0", f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]", "s_endpgm"]
    good = ["v_mov_b32_e32 v50, v1", "s_nop 1", f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]", "s_endpgm"]
    none = ["v_mov_b32_e32 v50, v1", "s_endpgm"]
    rep = ih.scan_listing(listing(("first", good), ("second", bad), ("third", none), ("fourth", bad[2:])))
    assert [(v.kernel, v.slot, v.states, v.consumer.addr) for v in rep.violations] == [("second", "B", 1, 0x1108)]
    assert (rep.kernels, rep.kernels_with_mfma, rep.mfmas, rep.producers) == (4, 3, 3, 2)
    assert rep.symbols == ["first", "second", "third", "fourth"]
    text = rep.format()
    assert "second" in text and "1108" in text and "v_mov_b32_e32 v50, v1" in text and "violations: 1" in text


def test_the_rule_is_a_table_row():
    (rule,) = ih.RULES
    assert rule.states == 2 and [s for _, s in rule.slots] == ["A", "B", "C"]
    three = ih.Rule(rule.name, rule.is_producer, rule.dests, rule.is_consumer, rule.slots, 3)
    txt = listing(("k", ["v_mov_b32_e32 v50, v1", "s_nop 1", f"{MFMA} v[92:95], v[54:57], v[50:53], v[66:69]", "s_endpgm"]))
    assert ih.scan_listing(txt).violations == [] and len(ih.scan_listing(txt, (three,)).violations) == 1


# ---- (b) end to end on a compiled fixture

def test_fixture_kernels_through_the_real_extraction(tmp_path):
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    obj = str(tmp_path / "hazard_fixture.o")
    subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-c",
                    os.path.join(ROOT, "tests", "hazard_fixture.hip"), "-o", obj], check=True)
    rep = ih.scan_file(obj)
    assert sorted(rep.symbols) == ["hazard_asm_pack", "hazard_visible_pack"] and rep.mfmas == 2
    assert rep.violations, "the asm pack one state in front of its MFMA was not found"
    for v in rep.violations:
        print(v.format())
        assert v.kernel == "hazard_asm_pack" and v.producer.mnemonic == "v_cvt_pk_bf16_f32" and v.slot == "A" and v.states < 2
    # the compiler-visible kernel holds the same instruction, padded
    assert rep.producers >= 8


# ---- (c) the library as built

@pytest.fixture(scope="module")
def library_report(pkg):
    return ih.scan_file(os.path.join(ROOT, "whisper.tflite_amd", "lib", "libwhisper-tflite.so"))


def test_library_has_no_valu_write_too_close_to_an_mfma(library_report):
    print(library_report.format())
    assert library_report.violations == [], library_report.format()


def test_library_scan_saw_the_kernels_it_is_there_for(library_report):
    rep = library_report
    assert rep.mfmas > 10000 and rep.producers > rep.mfmas
    for name in ("encoder_attention_planes", "dec_gemm", "cross_absorbed"):
        assert any(name in s for s in rep.symbols), name


def test_cli_reports_and_sets_its_exit_status(tmp_path, capsys):
    # a file that cannot be read is an extraction failure (2), not a clean report (0)
    assert ih.main([str(tmp_path / "missing.so")]) == 2
    assert "missing.so" in capsys.readouterr().err
