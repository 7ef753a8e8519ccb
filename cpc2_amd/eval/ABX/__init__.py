"""ABX within / across speakers (cpc/eval/ABX of the reference): item files, triplet iterators, batched DTW scoring."""
