/* cli_host.c -- the pieces the option parsers of the tools share: how an error
   is said, the arguments of an option as the reference's parser takes them
   (src/core/option.c), and the end of a parser loop.  Declared in
   host_internal.h; no tool's own options are here. */
#include "host_internal.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int gtamd_fail(char *err, size_t errlen, const char *msg, const char *arg)
{
  snprintf(err, errlen, msg, arg);
  return -1;
}

int gtamd_failf(char *err, size_t errlen, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, errlen, fmt, ap);
  va_end(ap);
  return -1;
}

int gtamd_opt_name(int argc, const char **argv, int *i, const char **name, char *err, size_t errlen)
{
  if (*i + 1 >= argc) return gtamd_fail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
  *name = argv[++*i];
  return 0;
}

int gtamd_opt_uint32(int argc, const char **argv, int *i, uint32_t *out, char *err, size_t errlen)
{
  char *end;
  unsigned long v;
  if (*i + 1 >= argc) return gtamd_fail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
  v = strtoul(argv[*i + 1], &end, 10);
  if (*end != 0 || argv[*i + 1][0] == '-')
    return gtamd_fail(err, errlen, "argument to option \"%s\" must be a non-negative integer", argv[*i]);
  *out = (uint32_t) v;
  (*i)++;
  return 0;
}

int gtamd_opt_length(int argc, const char **argv, int *i, unsigned long long max, unsigned long long *out,
                     char *err, size_t errlen)
{
  char *end;
  if (*i + 1 >= argc) return gtamd_fail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
  *out = strtoull(argv[*i + 1], &end, 10);
  if (*end != 0 || end == argv[*i + 1] || argv[*i + 1][0] == '-')
    return gtamd_fail(err, errlen, "argument to option \"%s\" is out of range", argv[*i]);
  if (*out < 1) return gtamd_fail(err, errlen, "argument to option \"%s\" must be an integer >= 1", argv[*i]);
  if (*out > max) return gtamd_fail(err, errlen, "argument to option \"%s\" is out of range", argv[*i]);
  (*i)++;
  return 0;
}

int gtamd_opt_files(int argc, const char **argv, int *i, const char *const **files, size_t *numfiles,
                    char *err, size_t errlen)
{
  const char *option = argv[*i];
  *files = argv + *i + 1;
  for (*numfiles = 0; *i + 1 < argc && argv[*i + 1][0] != '-'; (*i)++) (*numfiles)++;
  return *numfiles ? 0 : gtamd_fail(err, errlen, "missing argument to option \"%s\"", option);
}

int gtamd_opt_yesno(int argc, const char **argv, int *i)
{
  if (*i + 1 < argc && (!strcmp(argv[*i + 1], "yes") || !strcmp(argv[*i + 1], "no"))) {
    (*i)++;
    return !strcmp(argv[*i], "yes");
  }
  return 1;
}

int gtamd_opt_switch(int argc, const char **argv, int *i)
{
  if (*i + 1 < argc) {
    const char *v = argv[*i + 1];
    if (!strcmp(v, "yes") || !strcmp(v, "true")) { (*i)++; return 1; }
    if (!strcmp(v, "no") || !strcmp(v, "false")) { (*i)++; return 0; }
  }
  return 1;
}

int gtamd_opt_unsupported(const char *a, char *err, size_t errlen)
{
  return gtamd_fail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
}

int gtamd_opt_tail(const char *a, const char *const *refused, const char *unknown, const char *superfluous,
                   char *err, size_t errlen)
{
  for (int k = 0; refused != NULL && refused[k] != NULL; k++)
    if (!strcmp(a, refused[k])) return gtamd_opt_unsupported(a, err, errlen);
  return gtamd_fail(err, errlen, a[0] == '-' ? unknown : superfluous, a);
}
