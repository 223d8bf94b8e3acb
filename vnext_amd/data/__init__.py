"""The data side that stays on the host when the device does the pixels (clip_mapper.py)."""
