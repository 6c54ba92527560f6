"""Drop-in for the reference's model/DCNv2/dcn_v2_func.py (DCNv2Function and DCNv2PoolingFunction: forward, and backward through
autograd)."""
from m3dssd_amd.host.dcn import DCNv2Function, DCNv2PoolingFunction  # noqa: F401
