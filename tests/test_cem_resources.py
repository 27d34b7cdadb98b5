"""hipcc's resource report for the CEM planner's kernels (reagent_amd/csrc/cem.hip): the expected kernels, no scratch and no
spilled registers, and the rollout's LDS (static plus the launch's dynamic request) within the CU's 160 KB at the widest shape
it accepts."""
import reagent_amd._lib as L
from kernel_remarks import kernel_resources

EXPECTED = ["cem_fill_noise_kernel", "cem_group_kernel", "cem_rollout_kernel", "cem_ensemble_mean_kernel", "cem_sample_kernel",
            "cem_sample_discrete_kernel", "cem_refit_kernel", "cem_tally_kernel"]


def test_kernels_have_no_scratch_and_no_spills_and_the_rollout_fits_lds(tmp_path):
    kernels = kernel_resources("cem.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want in EXPECTED:
        hits = [k for k in kernels if want + "E" in k]
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 256, (want, v)
    static = [v for k, v in kernels.items() if "cem_rollout_kernelE" in k][0]["LDS Size [bytes/block]"]
    widest = L.load().rg_cem_rollout_lds_bytes(L.CEM_MAX_INPUT - 1, 1, L.LSTM_MAX_HIDDEN)
    assert widest == (32 * (L.CEM_MAX_INPUT + 1) + 2 * 32 * (L.LSTM_MAX_HIDDEN + 1)) * 4
    assert static + widest <= 160 * 1024, (static, widest)
