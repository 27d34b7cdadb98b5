"""hipcc's resource report for the world model's kernels (reagent_amd/csrc/lstm.hip, mdn.hip): the expected kernels, no
scratch and no spilled registers, LDS within the CU's 160 KB at the widest hidden size."""
import pytest

from kernel_remarks import kernel_resources

EXPECTED = {
    "lstm.hip": ["lstm_forward_kernel", "lstm_backward_kernel"],
    "mdn.hip": ["mdn_head_kernel", "mdn_finish_kernel", "mdn_nll_kernel", "mdn_outputs_kernel"],
}


@pytest.mark.parametrize("hip_file", sorted(EXPECTED))
def test_kernels_have_no_scratch_and_no_spills(tmp_path, hip_file):
    kernels = kernel_resources(hip_file, tmp_path)
    assert len(kernels) == len(EXPECTED[hip_file]), sorted(kernels)
    for want in EXPECTED[hip_file]:
        hits = [k for k in kernels if want in k]
        assert len(hits) == 1, (want, sorted(kernels))
        v = kernels[hits[0]]
        print(want, v)
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (want, v)
        assert v["VGPRs"] <= 256, (want, v)


def test_lstm_tiles_fit_lds_at_the_widest_hidden_size():
    """the dynamic LDS the two launches ask for at H = 256: two (forward) and three (backward) images of 32 x 257 floats"""
    image = 32 * (256 + 1) * 4
    assert 2 * image + 128 <= 160 * 1024 and 3 * image + 128 <= 160 * 1024
