// STAND-IN (empty): oracle/ref_shim/README.md
#pragma once
