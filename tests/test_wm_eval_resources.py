"""hipcc's resource report for the world-model evaluators' kernels (reagent_amd/csrc/wm_eval.hip): the expected kernels, no
scratch and no spilled registers, and the ablation kernel's dynamic LDS at H = 256 with the widest block within the CU's 160 KB."""
import reagent_amd._lib as L
from kernel_remarks import kernel_resources

# kernel -> the VGPRs recorded in profiles/NOTES_r34.md (a ceiling: more is a regression to look at)
EXPECTED = {"wm_feature_fill_kernel": 22, "lstm_ablate_kernel": 122, "wm_mdn_losses_kernel": 62, "wm_losses_finish_kernel": 14,
            "wm_sensitivity_kernel": 14, "wm_sensitivity_finish_kernel": 10}


def test_kernels_have_no_scratch_no_spills_and_fit_lds(tmp_path):
    kernels = kernel_resources("wm_eval.hip", tmp_path)
    assert len(kernels) == len(EXPECTED), sorted(kernels)
    for want, vgprs in EXPECTED.items():
        hits = [k for k in kernels if want + "E" in k]  # (the mangled name: ...<name>E...)
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= vgprs and v["LDS Size [bytes/block]"] <= 160 * 1024, (want, v)
    # two images of 32 x (H + 1) floats and the delta image of 32 x (width + 1), next to the kernel's static 128 bytes
    assert (2 * 32 * (L.LSTM_MAX_HIDDEN + 1) + 32 * (L.WM_MAX_BLOCK + 1)) * 4 + 128 <= 160 * 1024
