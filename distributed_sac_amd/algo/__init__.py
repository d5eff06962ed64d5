from .sac import SACEngine  # noqa: F401
from .care import CAREEngine  # noqa: F401


def create_engine(cfg, device="cpu", precision=None, max_grad_norm=None):
    """Variant dispatch: sac/vsac/mtsac -> SACEngine, care -> CAREEngine."""
    if cfg.variant == "care":
        return CAREEngine(cfg, device, precision=precision,
                          max_grad_norm=max_grad_norm)
    return SACEngine(cfg, device, precision=precision,
                     max_grad_norm=max_grad_norm)
