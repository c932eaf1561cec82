"""MI355X-native DiT denoisers of the cascaded image-to-3D and text-to-3D samplers (same class names, constructor arguments,
``forward`` / ``forward_with_cfg`` surfaces and state-dict keys as /root/reference/dit/dit_i23d.py and dit/dit_trilatent.py)."""
from .dit_i23d import (  # noqa: F401
    DiT_I23D_PCD_PixelArt_noclip,
    DiT_I23D_PCD_PixelArt_noclip_clay_stage2,
    DiT_models,
)
from .dit_trilatent import (  # noqa: F401
    DiT_PCD_PixelArt,
    DiT_PCD_PixelArt_tofeat,
)
from .dit_trilatent import DiT_models as DiT_models_t23d  # noqa: F401  (the reference imports the two registries under these names)
