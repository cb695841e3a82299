// Stand-in for the reference's generated config.h: only what its sources read.
#pragma once
#define VERSION "3.3.0"
