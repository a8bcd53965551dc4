"""GPU (-m gpu): every ``DL_*`` kernel-selection switch of the library (alternative kernels kept for comparison, forced variants, tuning knobs) must give the results
of the default path: the parity checks of tests/switch_probe.py (reference fixtures + oracle) run in a child process per switch -- most switches are read once per
process.  VERDICT r2: 33 getenv sites select kernels at run time and the suite exercised a few of them."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# (environment, sections of tests/switch_probe.py the switch can affect)
SWITCHES = [({}, 'fs two ens emu bao tns png mh stk tnsodd baoodd'),
            ({'DL_TNS_WAVEK': '0'}, 'tns tnsodd'), ({'DL_TNS_WAVEK': '1'}, 'tns tnsodd'),                                              # TNS loop kernel: split-K / one wavenumber per wave, whatever the batch
            ({'DL_TNS_W': '1'}, 'tnsodd'), ({'DL_TNS_W': '2'}, 'tns tnsodd'), ({'DL_TNS_W': '4'}, 'tns tnsodd'), ({'DL_TNS_W': '8'}, 'tnsodd'),   # ... every number of waves per wavenumber; tnsodd: table wavenumbers that leave waves without one (tests/theory_shapes_cases.py)
            ({'DL_NO_TOEPLITZ': '1'}, 'fs two png tnsodd'),                                        # general-knot spline solve (segmented Thomas) instead of the FIR form
            ({'DL_XCD_LOCAL': '0'}, 'fs emu'), ({'DL_XCD_LOCAL': '2', 'DL_CHI2_GEMM_MAX': '512'}, 'fs'),
            ({'DL_CHI2_GEMM_MAX': '512'}, 'fs two'),                                     # 2537 rows through the LDS-DMA GEMM with the partial-chi2 epilogue
            ({'DL_CHI2_GEMM_MAX': '512', 'DL_NO_CHI2_BIG': '1'}, 'fs two'),              # ... through the split-K slabs + slab finalize
            ({'DL_CHI2_GEMM_MAX': '512', 'DL_NO_CHI2_BIG': '1', 'DL_GEMM_DMA': '0'}, 'fs'),   # register-staged predecessor
            ({'DL_CHI2_GEMM_MAX': '512', 'DL_NO_CHI2_BIG': '1', 'DL_GEMM_WGS': '96'}, 'fs'),
            ({'DL_CHI2_GEMM_MAX': '4096'}, 'fs'),                                        # 2537 rows through the chi2 GEMM
            ({'DL_CG_MT': '16'}, 'fs two'), ({'DL_CG_MT': '32'}, 'fs two'),
            ({'DL_CHI2_BFRAG': '1'}, 'fs two ens mh'), ({'DL_CHI2_BFRAG': '1', 'DL_CG_MT': '16'}, 'fs two'),      # the chi2 GEMM with its B operand in registers (dl_chi2_gemm_tile_bf: round-6 experiment, measured slower, kept for the record)
            ({'DL_CHI2_FUSED': '1'}, 'fs'),
            ({'DL_STEP_KERNEL': '1'}, 'fs'),                                              # theory + chi2 GEMM + finalize of <= 1024 points in ONE launch (dl_step_kernel: measured slower, kept for the record)
            ({'DL_FS_WIDE': '0'}, 'fs'), ({'DL_FS_WIDE': '1'}, 'fs'),                     # the 512-thread theory kernel of small batches: never / whatever the batch
            ({'DL_FS_DENSE_MIN': '256'}, 'fs two'), ({'DL_FS_DENSE_MIN': '1000000'}, 'fs'),
            ({'DL_NO_MERGED_THEORY': '1'}, 'two ens'), ({'DL_NO_PANEL_SKIP': '1'}, 'two'), ({'DL_NO_ROW_ALIGN': '1'}, 'two ens'),
            ({'DL_ENS_GLOBAL': '1'}, 'ens'), ({'DL_ENS_NO_DEFER': '1'}, 'ens'), ({'DL_ENS_NO_FOLD': '1'}, 'ens'), ({'DL_MH_NO_DEFER': '1'}, 'mh'),
            ({'DL_NO_EMU_FUSED': '1'}, 'emu stk'), ({'DL_NO_GRAM_EPILOGUE': '1'}, 'emu stk'), ({'DL_NO_EMU_BATCH': '1'}, 'emu'), ({'DL_NO_FEATURE_PATH': '1'}, 'emu stk'),
            ({'DL_NO_FUSED_SOLVE': '1'}, 'emu stk'),
            ({'DL_NO_STK_SPLIT': '1'}, 'stk'),                                             # the stacked engine in one launch (dl_emulated_stacked_kernel: the round-5 form) instead of chains + feature GEMMs
            ({'DL_STK_OVERLAP': '1'}, 'stk'), ({'DL_STK_OVERLAP': '3'}, 'stk'), ({'DL_STK_OVERLAP': '4'}, 'stk'),   # dl_emulated_stacked_ov_kernel (round-6 experiment, measured slower, kept for the record): networks under the feature GEMM (3: no raised priority), split halves
            ({'DL_FM_NO_STAGE': '1'}, 'emu bao'),
            ({'DL_BAO_THREADS': '64'}, 'bao baoodd'), ({'DL_BAO_THREADS': '128'}, 'bao baoodd'), ({'DL_BAO_THREADS': '256'}, 'bao baoodd'),      # baoodd: 9 and 258 wavenumbers
            ({'DL_FFTLOG_GENERIC': '1'}, 'bao')]


def run_switch(item):
    env, sections = item
    out = subprocess.run([sys.executable, os.path.join(HERE, 'switch_probe.py')] + sections.split(), env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    return env, out.returncode, out.stdout.decode()[-300:], out.stderr.decode()[-1500:]


def test_every_kernel_selection_switch_reproduces_the_default_results():
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:      # four children share the GPU
        results = list(pool.map(run_switch, SWITCHES))
    failed = [(env, stderr) for env, code, stdout, stderr in results if code != 0 or 'switch probe ok' not in stdout]
    assert not failed, failed
