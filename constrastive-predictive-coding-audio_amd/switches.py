"""The environment switches the package still has, and the only module that reads the environment.  Each is set from outside the
package, some on a live engine, so every call reads the environment anew: no caching.  The retired A/B switches' numbers stand in
the comments beside the code they chose and in docs/DESIGN_HISTORY_r1-r3.md."""
import os


def wgrad_stream():
    """CPC_WGRAD_STREAM=0: weight-gradient GEMMs on the main stream.  Read by every backward pass of both engines; bench.py flips it on a live, warmed engine (roofline.alone), and a test sets it."""
    return os.environ.get("CPC_WGRAD_STREAM", "1") != "0"


def prepare_ahead():
    """CPC_PREPARE_AHEAD=0: operand copies not rebuilt behind the optimizer's update.  Read by every prepare_ahead() call of both engines; bench.py installs the hook that calls them by this name."""
    return os.environ.get("CPC_PREPARE_AHEAD", "1") != "0"


def preprocess_ahead():
    """CPC_PREPROCESS_AHEAD=0: preprocessing inside the step.  Read by the trainer's train() at every epoch; bench.py arranges its own loop by this name."""
    return os.environ.get("CPC_PREPROCESS_AHEAD", "1") != "0"


def fused_score():
    """CPC_FUSED_SCORE=0: the unfused score kernels.  Read by every fused_scores_ok() call; a test sets it on an engine that has already run a step."""
    return os.environ.get("CPC_FUSED_SCORE", "1") != "0"


def stem():
    """CPC_STEM=0: block 0 of a scalogram encoder without the stem kernels.  Read when a block is constructed; tests build both and compare."""
    return os.environ.get("CPC_STEM", "1") != "0"


def bn_residual():
    """CPC_BN_RESIDUAL=0: a block's last BatchNorm and its residual add as two passes.  Read by every forward pass of a block; tests run both and compare."""
    return os.environ.get("CPC_BN_RESIDUAL", "1") != "0"


def conv_gather():
    """CPC_CONV_GATHER, tri-state, the windowed convolutions without an im2col matrix: None (unset) for bf16 only, True ("1") also for the
    float32 forward, False ("0") off.  Read when a convolution is constructed; tests build the model with each setting and compare."""
    return {"1": True, "0": False}.get(os.environ.get("CPC_CONV_GATHER"))


def bn_bias_colsum():
    """CPC_BN_BIAS_COLSUM=1: the bias gradient in front of a train-mode BatchNorm (zero by construction) summed as the reference's autograd
    does, instead of written as zero.  Read by every backward pass of such a convolution; a documented user option."""
    return os.environ.get("CPC_BN_BIAS_COLSUM", "0") == "1"
