__all__ = ["InterleavedOutput"]


def __getattr__(name):
    # resolved on first use: `import dreamllm_amd` (e.g. for `dreamllm_amd.build`) stays free of torch
    if name == "InterleavedOutput":
        from .generation import InterleavedOutput
        return InterleavedOutput
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
