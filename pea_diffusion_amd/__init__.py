# (no re-exports: import the submodule you need).  The one thing that must happen as early as possible -- before the HIP
# runtime initialises -- is the launch configuration the package is measured in; see _lib.py.
# Runtime switches of a UNet context live on unet.HipUNet: enable_freeu / disable_freeu, set_ip_tokens, set_inpaint_cond, ...
import os as _os

_os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
