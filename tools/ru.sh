#!/bin/bash
# ru.sh [extra flags] -- resource usage (VGPRs, scratch, spills) of the KSheba instantiation of the step kernel with the product
# flags: `make resource-usage` of samsim_amd/csrc (WAVES from the environment, as the Makefile takes it), filtered
make -C "$(dirname "$0")/../samsim_amd/csrc" resource-usage EXTRA="$*" 2>&1 | grep -E "error|Function Name|VGPRs:|Scratch|Spill" | sed 's/.*remark: //' | cut -c1-100 | grep -E -A4 "error|samsim_step_kernelINS_6KShebaE"
