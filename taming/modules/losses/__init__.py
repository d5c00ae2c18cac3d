"""`taming.modules.losses.DummyLoss` (lossconfig.target of every shipped first-stage config), the LPIPS perceptual metric and the
tokenizer's full loss."""
from frido_amd.models import DummyLoss, LPIPS, VQLPIPSWithDiscriminator  # noqa: F401
