from .dataset import BubbleForecast, DeviceClipStore, Q16ClipStore  # noqa: F401
