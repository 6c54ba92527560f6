"""Drop-in for the reference's lib/loss/rpn_3d.py (``from lib.loss.rpn_3d import *``)."""
from m3dssd_amd.host.loss import RPN_3D_loss, RPN_3D_loss_smp  # noqa: F401

__all__ = ["RPN_3D_loss", "RPN_3D_loss_smp"]
