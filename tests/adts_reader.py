"""A strict ADTS reader for the audio-tap tests, written from the header layout alone (ISO/IEC
13818-7 / 14496-3 adts_frame without CRC).  It shares no code with tests/aac_model.py.

fixed header:    syncword 12 bits (FFF), ID 1, layer 2 (00), protection_absent 1, profile 2,
                 sampling_frequency_index 4, private 1, channel_configuration 3, original 1, home 1
variable header: copyright id bit 1, copyright id start 1, aac_frame_length 13, adts_buffer_fullness
                 11, number_of_raw_data_blocks_in_frame 2
"""


class AdtsError(ValueError):
    pass


def read(data: bytes):
    """-> (profile, frequency index, channels, [frame body bytes]).  The frame lengths must tile the
    file exactly, and profile, frequency and channels must be the same in every header."""
    at, frames, fixed = 0, [], None
    while at < len(data):
        if len(data) - at < 7:
            raise AdtsError(f"{len(data) - at} stray bytes at {at}")
        h = int.from_bytes(data[at:at + 7], "big")
        if h >> 44 != 0xFFF:
            raise AdtsError(f"no syncword at {at}")
        if (h >> 41) & 3:
            raise AdtsError(f"layer is not 0 at {at}")
        if not (h >> 40) & 1:
            raise AdtsError(f"protection_absent is 0 at {at}: a CRC would follow")
        this = ((h >> 38) & 3, (h >> 34) & 15, (h >> 30) & 7)
        if fixed is None:
            fixed = this
        elif this != fixed:
            raise AdtsError(f"profile / frequency / channels change at {at}: {fixed} -> {this}")
        length = (h >> 13) & 0x1FFF
        if length < 7 or at + length > len(data):
            raise AdtsError(f"frame length {length} at {at} does not fit {len(data)} bytes")
        if h & 3:
            raise AdtsError(f"more than one raw data block at {at}")
        frames.append(bytes(data[at + 7:at + length]))
        at += length
    if fixed is None:
        return None, None, None, []
    return fixed[0], fixed[1], fixed[2], frames
