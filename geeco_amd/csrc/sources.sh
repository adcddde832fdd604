# The .hip translation units of libgeeco_hip.so and their compiler flags: sourced by build.sh and by scripts/dev/build_variant.sh
# and build_stamps.sh, so a file is added or split in one place.
HIP_SOURCES="conv_gemm conv_halo_conv1 conv_halo_s2_fwd conv_halo_s2_bwd conv_halo_bottom conv_wgrad conv_wgrad_halo conv_dgrad_lds dynimg dynimg_goal input_grad frame_pack window_gather decoder_concat decoder_gemm decoder_lstm decoder_heads decoder_step_bwd decoder_seq misc adam grad_accum clip guard varstats lr_schedule predict_io shared_frames replay replay_dynimg attribution perturbation"
BASE_FLAGS="-O3 --offload-arch=gfx950 -fPIC -std=c++17"      # errors.cpp (no kernels) is compiled with these
WARN_FLAGS="-Wall -Wno-unused-function"                    # the product and variant builds; build_stamps.sh leaves them out
# -amdgpu-mfma-vgpr-form: accumulators stay in VGPRs (unified file on gfx950); without it the allocator parks them in AGPRs in
# some kernels and pays v_accvgpr_read/write copies, each of which costs MFMA issue time
KERNEL_FLAGS="$BASE_FLAGS -mllvm -amdgpu-mfma-vgpr-form"
FLAGS="$KERNEL_FLAGS $WARN_FLAGS"
# per-file scheduler settings (same-box A/B of whole-library variants, per-layer table: profiles/r03/ab_compiler_flags.txt):
# the gather GEMM gains 2-3 % from the max-ILP strategy (conv4-6 forward), the LDS-halo and LDS-staged input-gradient
# kernels 0.5-1 % from the AMDGPU register-pressure trackers; every other combination measured was neutral or worse
extra_flags() {
  case $1 in
    conv_gemm) echo "-mllvm -amdgpu-sched-strategy=max-ilp" ;;
    conv_halo_*|conv_dgrad_lds) echo "-mllvm -amdgpu-use-amdgpu-trackers=1" ;;
  esac
}
