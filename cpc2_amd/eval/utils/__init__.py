"""File-to-file tools of the reference's cpc/eval/utils: adjust_sample_rate (bring a corpus to one sample rate)."""
