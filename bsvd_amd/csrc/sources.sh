# The translation units of libbsvd_hip.so, stated once: sourced by build.sh, tools/isa_digest.sh and tools/kernel_resources.sh.
# A measurement build (EXTRA_HIPCC_FLAGS contains -DBSVD_MEASURE, tools/build_measure.sh) adds conv3x3_wino.hip (the rejected
# all-positions-per-wave Winograd kernel) and the variant instantiations of conv3x3_winox.hip.
BSVD_SRCS="conv3x3_mfma conv3x3_winox conv3x3_edge_f32 bsvd_abi weight_pack tensor_layout frame_yuv frame_rgb frame_sigma frame_scene frame_finish frame_nlf frame_vst frame_grain"
case " ${EXTRA_HIPCC_FLAGS} " in *" -DBSVD_MEASURE"*) BSVD_SRCS="$BSVD_SRCS conv3x3_wino";; esac
# per-source flags.  conv3x3_winox: no SLP vectorizer (it turns the transform's fma_mix forms into convert + packed-fp32 math, see dec_pair);
# frame_sigma, frame_rgb, frame_finish, frame_nlf, frame_vst, frame_grain: no contraction (the estimate / the code arithmetic / the blend / the noise map / the transform / the grain model are defined operation by operation, frame_sigma_items.h, bsvd_hip.h)
bsvd_src_flags() { case "$1" in conv3x3_winox) echo "-fno-slp-vectorize";; frame_grain|frame_sigma|frame_rgb|frame_finish|frame_nlf|frame_vst) echo "-ffp-contract=off";; esac; }
