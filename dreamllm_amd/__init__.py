__all__ = ["InterleavedOutput", "HipCLIPModel", "HipCLIPTextModel", "ClipSelection", "BestOfNOutput"]


def __getattr__(name):
    # resolved on first use: `import dreamllm_amd` (e.g. for `dreamllm_amd.build`) stays free of torch
    if name in ("InterleavedOutput", "BestOfNOutput"):
        from . import generation
        return getattr(generation, name)
    if name in ("HipCLIPModel", "HipCLIPTextModel", "ClipSelection"):
        from . import clip_model
        return getattr(clip_model, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
