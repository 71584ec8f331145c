"""MI355X-native implementation of the LearningByCheating sensorimotor training hot path.

Drop-in boundary = the reference's module API:
    from learningbycheating_amd.bird_view.models.image import ImagePolicyModelSS
    from learningbycheating_amd.bird_view.models.birdview import BirdViewPolicyModelSS
Per-step compute runs in hand-written HIP kernels for gfx950 (csrc/), reached through the
C ABI of include/lbc_hip.h; torch only provides device memory, streams and RCCL.
"""
__version__ = "0.1.0"

#: Declared accuracy of the precision modes (asserted by tests/test_model.py::test_bf16_mode_declared_accuracy on the MI355X
#: and quoted next to `dtype` in bench.py's JSON line).  Waypoints are normalised coordinates in [-1, 1].
#:   fp32: exact-f32 MFMA everywhere -- the north-star bar (|waypoint - reference PyTorch-CPU forward| <= 1e-3), asserted at 1e-4.
#:   bf16: BASELINE.json config 3 (bf16 MFMA operands + bf16 activation storage, f32 master weights / accumulate / BN / loss /
#:         Adam) on a trained-like (warm-started, calibrated) network: max |waypoint - fp32 executor| <= 3e-2 and mean <= 4e-3
#:         (measured on MI355X, r34 160x384 batch 32: eval mode max 1.1e-2 / mean 1.1e-3, training mode -- batch statistics
#:         move too -- max 2.2e-2 / mean 2.6e-3; profiles/r02_grad_diag.txt).  The yardstick is the REFERENCE arithmetic in bf16:
#:         the oracle under torch.autocast(bfloat16) on the same network and batch deviates max 2.7e-2 / mean 2.7e-3 from its own
#:         f32 forward, and its gradients sit at the same distance from the float64 gradients as the executor's (median 3.3e-2 of
#:         each tensor's largest entry both, cosine 0.9995 both; profiles/r03_run10_bf16_grad_vs_autocast.txt,
#:         tests/test_model.py::test_bf16_gradients_match_autocast_reference) -- the tolerance is what bf16 costs, not what this
#:         implementation adds; bf16 cannot meet 1e-3.
#:   bf16x3: split-bf16 convolution operands (hi*hi + hi*lo + lo*hi on the bf16 MFMA, f32 tensors; stem, BatchNorm, head, loss and
#:         Adam exact f32): the north-star bar, max <= 1e-3 and mean <= 1e-4 against the f32 oracle (measured on MI355X at batch 256:
#:         r34 160x384 eval max 4.2e-4 / mean 2.8e-5, train 5.6e-4 / 2.4e-5; r18 bird-view max 1.5e-4 / mean 8.9e-6;
#:         tests/test_precision_bf16x3.py::test_bf16x3_forward_parity_at_bench_batch_256).
WAYPOINT_TOLERANCE = {"fp32": 1e-3, "bf16": 3e-2, "bf16_mfma": 3e-2, "bf16x3": 1e-3}
#: ... and the mean absolute deviation over all predicted waypoint coordinates of a batch
WAYPOINT_MEAN_TOLERANCE = {"fp32": 1e-4, "bf16": 4e-3, "bf16_mfma": 4e-3, "bf16x3": 1e-4}
