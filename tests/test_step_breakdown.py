"""tools/step_breakdown.py on a synthetic rocpd database: the kernel names are the ones a kernel trace of the plain
benchmark holds (MIOpen / CK convolutions, torch's elementwise passes, Tensile GEMMs, this library), the windows are
bounded by the once-per-frame warp launch, and what runs before them (find phase, calibration) stays out."""
import os
import sqlite3
import subprocess
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

CONV = ["igemm_fwd_gtcx35_nhwc_fp32_bx0_ex1_bt128x64x16_wt32x32x2_ws1x1_wr1x2_ta1x8x1x1_1x2x4x32_tb1x4x1x1_1x2x1x128.kd",
        "_ZN2ck16tensor_operation6device12_GLOBAL__N_149kernel_grouped_conv_fwd_multiple_abd_xdl_cshuffleINS_1EEvT_",
        "miopenSp3AsmConv_v30_3_1_gfx9_fp32_f2x3_stride1.kd"]
ELEMENTWISE = ["MIOpenBatchNormFwdInferSpatialEst.kd", "SubTensorOpWithScalar1d.kd", "batched_transpose_32x32_dword.kd",
               "void at::native::vectorized_elementwise_kernel<4, at::native::(anonymous namespace)::launch_clamp_scalar(at::TensorIteratorBase&, "
               "c10::Scalar, c10::Scalar, at::native::detail::ClampLimits)::{lambda()#1}::operator()() const::{lambda()#7}::operator()() const::"
               "{lambda(float)#1}, std::array<char*, 2ul> >(int, float, std::array<char*, 2ul>)",
               "void at::native::vectorized_elementwise_kernel<4, at::native::CUDAFunctor_add<float>, std::array<char*, 3ul> >(int, "
               "at::native::CUDAFunctor_add<float>, std::array<char*, 3ul>)",
               "void at::native::(anonymous namespace)::max_pool_forward_nhwc<float, float>(float const*, int, long, long, long)",
               "void at::native::elementwise_kernel_manual_unroll<128, 4, at::native::gpu_kernel_impl_nocast<at::native::direct_copy_kernel_cuda("
               "at::TensorIteratorBase&)::{lambda()#3}::operator()() const::{lambda()#7}::operator()() const::{lambda(float)#1}>(at::TensorIteratorBase&)::"
               "{lambda(int)#1}>(int, float)",
               "void mvdetr::bn_act_cl<1, true>(float const*, mvdetr::BnVectors, float const*, mvdetr::BnVectors, long, int, int, float*)",
               "void mvdetr::bn_relu_maxpool_cl<int>(float const*, mvdetr::BnVectors, int, int, int, int, int, int, int, float*)"]
GEMM = ["Cijk_Alik_Bljk_S_B_Bias_HA_S_SAV_UserArgs_MT96x192x16_MI16x16x1_SN_LDSB1_AFC1.kd", "Cijk_Ailk_Bljk_SB_MT128x128x32_MI16x16x4x1_SN.kd"]
OURS = ["void mvdetr::msda_fwd_group2<mvdetr::TileCfg<16, 32, 6, 16, 6, 256, 6>, 7, 2, 2>(mvdetr::FusedArgs)",
        "void mvdetr::add_layernorm_rows128x2(float const*, float const*, float*)"]
MARK = "void mvdetr::warp_fwd_cl<float>(float const*, float const*, int, int, float*)"


def test_groups_and_short_names():
    import step_breakdown as sb
    for names, group in ((CONV, 0), (ELEMENTWISE, 1), (OURS + [MARK], 2), (GEMM, 3), (["some_other_kernel"], 4)):
        for n in names:
            assert sb.group_of(n) == sb.GROUPS[group], n
    assert sb.short(ELEMENTWISE[5]) == "max_pool_forward_nhwc<float, float>"
    assert sb.short(ELEMENTWISE[3]).startswith("vectorized_elementwise_kernel<4, launch_clamp_scalar")
    assert sb.short(ELEMENTWISE[7]) == "mvdetr::bn_act_cl<1, true>" and sb.short(CONV[2]) == CONV[2]


def test_windows_hold_whole_frame_periods_and_skip_the_start_of_the_process(tmp_path):
    db = str(tmp_path / "t.db")
    con = sqlite3.connect(db)
    con.execute("create table kernels(name, start, duration)")
    t = 0
    for _ in range(500):                                         # a find phase: trial launches, no marker
        con.execute("insert into kernels values(?,?,?)", ("naive_conv_fwd_nchw.kd", t, 7_000_000))
        t += 7_001_000
    frame = [(CONV[0], 2_000_000), (ELEMENTWISE[0], 40_000), (ELEMENTWISE[7], 60_000), (MARK, 30_000), (OURS[0], 100_000), (GEMM[0], 50_000),
             (CONV[1], 200_000)]
    for _ in range(8):
        for name, dur in frame:
            con.execute("insert into kernels values(?,?,?)", (name, t, dur))
            t += dur + 2_000
    con.commit()
    con.close()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "step_breakdown.py"), db, "--frames", "5"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert "5 frame periods between the last 6 launches of warp_fwd_cl (8 in the trace)" in lines[0]
    assert "per frame: 7.0 launches, 2480.0 us of kernel time, 2494.0 us from marker to marker" in lines[1]
    rows = {l[:32].strip(): l[32:].split() for l in lines[3:8]}
    assert rows["convolutions (MIOpen / CK)"][:2] == ["2.0", "2200.0"] and rows["elementwise passes"][:2] == ["2.0", "100.0"]
    assert rows["this library"][:2] == ["2.0", "130.0"] and rows["GEMMs"][:2] == ["1.0", "50.0"] and rows["other"][:2] == ["0.0", "0.0"]
    assert not any("naive_conv" in l for l in lines)
