"""Shared by tests/golden/make_golden_edit.py and the editing tests: the runs of the reference's own mask / x0 blend that are recorded in
edit_ref.npz.  The reference's blend (ddim.py:158-161) only executes where the state carries x0's channels: the two-stage model with x_T
given, so that stage 0 is adopted and stage 1 runs with all 6 channels."""
B, SHAPE, S, NUM_STAGE = 2, (6, 16, 16), 4, 2
# name -> (eta, mask kind)
RUNS = {"eta0_binary": (0.0, "binary"), "eta1_binary": (1.0, "binary"), "eta0_soft": (0.0, "soft"), "eta1_soft": (1.0, "soft")}
