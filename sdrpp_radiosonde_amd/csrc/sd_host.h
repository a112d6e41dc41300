// sd_host.h -- what a pure-host source of the library needs from batch.hip: the error message behind sonde_last_error()
#pragma once
int sd_fail_msg(const char *what);      // records the message, returns -1
