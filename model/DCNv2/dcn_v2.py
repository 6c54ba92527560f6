"""Drop-in for the reference's model/DCNv2/dcn_v2.py (DCNv2, DCN, DCNv2Pooling, DCNPooling)."""
from m3dssd_amd.host.dcn import DCNv2, DCN, DCNv2Function  # noqa: F401
from m3dssd_amd.host.dcn import DCNv2Pooling, DCNPooling, DCNv2PoolingFunction  # noqa: F401
